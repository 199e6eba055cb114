"""GPU: the overlay kernels (csrc/overlay.hip) through the C ABI and the wrappers of utils/utils_ipn.py against the numpy restatement
of tests/overlay_ref.py and the pictures recorded from the reference (tests/golden/overlay_fixtures.npz).  Every comparison is bit for
bit: the styles are integer work and float64 blends rounded operation by operation, which numpy reproduces exactly.

Every buffer lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.  The vector and the scalar
kernels are both run by the case table (odd widths and one-element pointer offsets take the scalar ones) and once more against each
other with IVOSW_OVERLAY_SCALAR=1 in a fresh child process."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import utils_ipn
from tests import overlay_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "overlay_fixtures.npz")
PAD = 16                                                  # elements in front of and behind every buffer: a multiple of 16 bytes for each type
SIZES = [(1, 1), (2, 7), (5, 5), (9, 33), (17, 64), (33, 70), (3, 6), (7, 854)]      # widths % 4: 0 (4 pixels a lane), 2 (2 pixels), odd (1)
OUT_FILL = 0xA5
X_IN = 99                                                 # byte 3 of the RGBX8 frames handed in: the pictures' byte 3 must come out 0 all the same
KINDS = {"rgbx": L.FRAMES_RGBX8, "f32": L.FRAMES_F32}
OUTS = {"rgb": L.OUT_RGB8, "rgbx": L.OUT_RGBX8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _vector_path_unless_asked(monkeypatch):
    monkeypatch.delenv("IVOSW_OVERLAY_SCALAR", raising=False)


class Buf:
    """A device buffer holding `data` (flat) PAD + off elements inside an allocation filled with `fill`; `ptr()` addresses the data;
    `back()` returns the data as it is now after checking the guard bands."""

    def __init__(self, dev, data, fill, off=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.lo, self.n = PAD + off, data.size
        self.host = np.full(data.size + 3 * PAD, fill, data.dtype)
        self.host[self.lo:self.lo + self.n] = data
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.lo * self.t.element_size())

    def back(self, name, unchanged=False):
        h = self.t.cpu().numpy()
        bits = lambda a: a.view(np.uint8)
        assert (bits(h[:self.lo]) == bits(self.host[:self.lo])).all() and (bits(h[self.lo + self.n:]) == bits(self.host[self.lo + self.n:])).all(), \
            f"{name}: written outside its extent"
        if unchanged:
            np.testing.assert_array_equal(bits(h), bits(self.host), err_msg=f"{name}: written by a refused call / an input")
        return h[self.lo:self.lo + self.n]


def images(n, H, W, seed=0):
    rng = np.random.default_rng(31 * H + W + seed)
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    img[:, H // 2, : W // 2 + 1] = 255
    img[:, H // 2, W // 2 + 1:] = 0
    return img


def label_maps(n, H, W, n_objects):
    """n label maps with a sparse random rest (0 .. n_objects + 1), two objects touching (zero pixels apart) and two one pixel apart,
    values above n_objects next to them, and objects in every corner and on all four borders."""
    rng = np.random.default_rng(1000 * H + 10 * W + n_objects)
    lab = np.where(rng.random((n, H, W)) < 0.08, rng.integers(0, n_objects + 2, (n, H, W)), 0).astype(np.uint8)
    A, B, C = 1, min(2, n_objects), n_objects
    above = (n_objects + 1, 255, 254, 128 if n_objects < 128 else 255)
    for k in range(n):
        m = lab[k]
        if H >= 5 and W >= 5:
            y, x = H // 2, W // 2
            m[y - 2:y + 3, max(x - 3, 0):x + 3] = 0
            m[y - 1:y + 1, x - 2:x] = A                                   # A and C side by side: zero pixels apart
            m[y - 1:y + 1, x:x + 2] = C
            m[y + 2, x - 2] = B                                           # one pixel of nothing between A and B
            m[y + 1, x + 1] = above[k % 4]                                # no object, below C
        if H >= 9:
            m[1, 2:6] = above
        m[0, 0], m[0, W - 1], m[H - 1, 0], m[H - 1, W - 1] = A, C, B, A   # corners
        m[0, W // 2], m[H - 1, W // 2], m[H // 2, 0], m[H // 2, W - 1] = B, A, C, B                            # borders
    if H == 1 and W == 1 and n > 1:
        lab[1:] = 0                                                       # a map with nothing in it
    return lab


def planes_of(img):
    """u8 / 255 as float32 [n,3,H,W]: the floats whose image bytes are the bytes themselves."""
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def options(style, n_objects, select=0, alpha=0.5, palette=None, color=(255, 0, 255)):
    return utils_ipn.overlay_options(style, n_objects, select, alpha, palette, color)


def render(dev, frames, lab, opt, kind="rgbx", out="rgb", ids=None, off=(0, 0, 0), geom=None):
    """One ivosw_overlay_frames call on guarded buffers.  frames: uint8 [n,H,W,3] images (kind "rgbx": packed with byte 3 = X_IN;
    "f32": as u8 / 255) or, for "f32", float32 [n,3,H,W] planes.  off: element offsets of (frames, labels, out) - uint32 / float32,
    uint8, and uint8 (RGB8) or uint32 (RGBX8) elements.  geom overrides arguments.  -> (rc, pictures, buffers)."""
    n, H, W = lab.shape
    if kind == "rgbx":
        fdata = np.concatenate([frames, np.full(frames.shape[:3] + (1,), X_IN, np.uint8)], 3).view(np.uint32)
        ffill = 0x01010101
    else:
        fdata = frames if frames.dtype == np.float32 else planes_of(frames)
        ffill = np.float32(0.5)
    m = n if ids is None else len(ids)
    odata = np.full(m * H * W * (4 if out == "rgbx" else 3), OUT_FILL, np.uint8)
    ofill = OUT_FILL
    if out == "rgbx":
        odata, ofill = odata.view(np.uint32), OUT_FILL * 0x01010101
    fb, lb, ob = Buf(dev, fdata, ffill, off[0]), Buf(dev, lab, 1, off[1]), Buf(dev, odata, ofill, off[2])     # label guard: an object that WOULD show
    g = dict(frames=fb.ptr(), frames_kind=KINDS[kind], labels=lb.ptr(), n_frames=n, H=H, W=W, ids=None if ids is None else L.int_array(ids),
             n_ids=m, opt=ctypes.byref(opt) if opt is not None else None, out=ob.ptr(), out_kind=OUTS[out])
    g.update(geom or {})
    rc = L.lib().ivosw_overlay_frames(g["frames"], g["frames_kind"], g["labels"], g["n_frames"], g["H"], g["W"], g["ids"], g["n_ids"],
                                      g["opt"], g["out"], g["out_kind"], L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    fb.back("frames", unchanged=True)
    lb.back("labels", unchanged=True)
    pics = ob.back("out", unchanged=rc != 0).view(np.uint8).reshape(m, H, W, 4 if out == "rgbx" else 3)
    return rc, pics, (fb, lb, ob)


def check(dev, img, lab, style, n_objects, kind="rgbx", out="rgb", ids=None, off=(0, 0, 0), why="", lanes=None, **kw):
    """One call against the restatement.  lanes: the pixels per lane the launcher must choose for these buffers (None: not asserted)."""
    want = R.overlay(img, lab, style, n_objects, frame_ids=ids, out=out, **kw)
    rc, got, (fb, lb, ob) = render(dev, img, lab, options(style, n_objects, **kw), kind, out, ids, off)
    assert rc == 0, L.lib().ivosw_last_error()
    if lanes is not None:
        assert L.lib().ivosw_overlay_lane_pixels(fb.ptr(), lb.ptr(), lab.shape[2], ob.ptr(), OUTS[out]) == lanes, (why, off, kind, out)
    np.testing.assert_array_equal(got, want, err_msg=f"{why} {style} n_objects={n_objects} {kind}->{out} {kw} off={off}")
    return got


# ================================================================================================ the case table
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_case_table(dev, H, W):
    n = 2
    img = images(n, H, W)
    for n_objects in (1, 3, 32):
        lab = label_maps(n, H, W, n_objects)
        for select in (0, n_objects):
            for style in R.STYLES:
                kw = dict(select=select, alpha=0.3 if n_objects == 3 else 0.5, color=(3, 250, 9) if select else (255, 0, 255))
                for kind in KINDS:
                    for out in OUTS:
                        got = check(dev, img, lab, style, n_objects, kind, out, why=f"{H}x{W}", lanes=4 if W % 4 == 0 else 2 if W % 2 == 0 else 1, **kw)
                        assert out == "rgb" or (got[..., 3] == 0).all()


def test_scalar_kernel_by_pointer_offset(dev):
    """W % 4 == 0, but one buffer at a time sits one element (the scalar kernel) or two (the 2-pixel kernel) off the grid the 4-pixel
    kernel needs."""
    H, W, n_objects = 17, 64, 3
    img, lab = images(2, H, W), label_maps(2, H, W, 3)
    for style in R.STYLES:
        for kind in KINDS:
            for out in OUTS:
                for off, lanes in (((1, 0, 0), 1), ((0, 1, 0), 1), ((0, 0, 1), 1), ((3, 2, 1), 1), ((2, 0, 0), 2), ((0, 2, 0), 2), ((0, 0, 2), 2),
                                   ((2, 2, 2), 2), ((4, 4, 4), 4), ((2, 1, 0), 1)):
                    check(dev, img, lab, style, n_objects, kind, out, off=off, alpha=0.3, lanes=lanes)


def test_scalar_env_in_this_process(dev, monkeypatch):
    H, W = 17, 64
    img, lab = images(2, H, W), label_maps(2, H, W, 3)
    monkeypatch.setenv("IVOSW_OVERLAY_SCALAR", "1")        # read by the launcher at every call
    for style in R.STYLES:
        check(dev, img, lab, style, 3, "rgbx", "rgb", lanes=1)
        check(dev, img, lab, style, 3, "f32", "rgbx", lanes=1)


# ================================================================================================ frame lists
def test_frame_lists(dev):
    H, W, n = 9, 32, 5
    img, lab = images(n, H, W), label_maps(n, H, W, 3)
    for ids in (None, [4, 3, 2, 1, 0], [2, 2, 0, 4, 2, 0], [3]):
        for kind, out in (("rgbx", "rgb"), ("f32", "rgbx")):
            check(dev, img, lab, "davis", 3, kind, out, ids=ids, why=f"ids={ids}")
            check(dev, img, lab, "fade", 3, kind, out, ids=ids, why=f"ids={ids}")
    H, W = 8, 33                                           # and on the scalar kernel
    img, lab = images(n, H, W), label_maps(n, H, W, 3)
    check(dev, img, lab, "davis", 3, ids=[4, 0, 0, 3])


def test_more_frames_than_one_launch_takes(dev):
    """300 frames of 2 x 8: the frame ids travel in the kernel arguments, 256 to a launch."""
    n, H, W = 300, 2, 8
    img, lab = images(n, H, W), label_maps(n, H, W, 3)
    lab[:, 0, 3] = np.arange(n) % 4                        # every frame its own picture
    img[:, 1, 5, 0] = np.arange(n) % 251
    for kind, out in (("rgbx", "rgb"), ("f32", "rgbx")):
        check(dev, img, lab, "davis", 3, kind, out)
        check(dev, img[:7], lab[:7], "fade", 3, kind, out, ids=[(5 * j) % 7 for j in range(300)])
    check(dev, img, lab, "checker", 3, off=(0, 1, 0), ids=list(range(299, -1, -1)))


# ================================================================================================ the byte rule of float frames
def test_float_frames_follow_the_byte_rule(dev):
    H, W = 9, 32
    rng = np.random.default_rng(5)
    f = rng.random((2, 3, H, W), dtype=np.float32) * np.float32(1.6) - np.float32(0.3)          # below 0 and above 1 among them
    specials = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0000001, -1e-9, 0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, 255.4 / 255,
                255.5 / 255, 256.0 / 255, 1e30, -1e30, 1e-40, 0.49999997 / 255]
    f[0, 0, 0, :len(specials)] = specials
    f[1, 2, H - 1, :len(specials)] = specials[::-1]
    img = R.frame_bytes(f)
    assert img[0, 0, 0, 0] == 0 and img[0, 0, 2, 0] == 255 and img[0, 0, 3, 0] == 0 and img.min() == 0 and img.max() == 255
    np.testing.assert_array_equal(R.frame_bytes(planes_of(images(1, H, W))), images(1, H, W))   # u8 / 255 gives u8 back
    lab = label_maps(2, H, W, 3)
    for style in R.STYLES:
        for off in ((0, 0, 0), (1, 0, 0)):
            want = R.overlay(img, lab, style, 3)
            rc, got, _ = render(dev, f, lab, options(style, 3), "f32", "rgb", off=off)
            assert rc == 0, L.lib().ivosw_last_error()
            np.testing.assert_array_equal(got, want, err_msg=f"{style} off={off}")


# ================================================================================================ the recorded pictures
def _gold_cases():
    g = np.load(GOLD)
    pal1 = lambda rgb: [rgb]
    for H, W in g["sizes"]:
        key = f"{H}x{W}_"
        img, lab = g[key + "image"][None], g[key + "label"][None]
        for a in (0.5, 0.3):
            yield img, lab, g[key + f"davis_a{a}"], "davis", 1, dict(select=1, alpha=a, palette=pal1((255, 0, 0)))
            yield img, lab, g[key + f"davis_rgb_a{a}"], "davis", 3, dict(select=1, alpha=a, palette=pal1((10, 201, 77)))
            yield img, lab, g[key + f"davis_seq_a{a}"], "davis", 3, dict(select=0, alpha=a)
            yield img, lab, g[key + f"davis_obj2_a{a}"], "davis", 3, dict(select=2, alpha=a)
        yield img, lab, g[key + "fade"], "fade", 1, dict(select=1)
        yield img, lab, g[key + "checker"], "checker", 3, dict(select=1)
        yield img, lab, g[key + "color"], "color", 3, dict(select=1)
        yield img, lab, g[key + "color_rgb"], "color", 3, dict(select=1, color=(3, 250, 9))


def test_goldens_through_the_c_abi(dev):
    assert tuple(np.load(GOLD)["palette3"].reshape(-1)) == tuple(R.davis_palette(3).reshape(-1))
    for img, lab, want, style, n_objects, kw in _gold_cases():
        for kind in KINDS:
            got = check(dev, img, lab, style, n_objects, kind, "rgb", why="golden", **kw)
            np.testing.assert_array_equal(got[0], want, err_msg=f"golden {style} {kw}")


def test_drop_in_wrappers_reproduce_the_goldens(dev):
    g = np.load(GOLD)
    for H, W in g["sizes"]:
        key = f"{H}x{W}_"
        img, lab = g[key + "image"], g[key + "label"]
        keep = img.copy()
        for a in (0.5, 0.3):
            np.testing.assert_array_equal(utils_ipn.overlay_davis(img, lab, alpha=a), g[key + f"davis_a{a}"])
            np.testing.assert_array_equal(utils_ipn.overlay_davis(img, lab.astype(np.float64), rgb=[10, 201, 77], cscale=7, alpha=a), g[key + f"davis_rgb_a{a}"])
            np.testing.assert_array_equal(utils_ipn.overlay_davis(img, lab == 2, rgb=[0, 128, 0], alpha=a), g[key + f"davis_obj2_a{a}"])
        got = utils_ipn.overlay_davis(img, lab)
        assert got.dtype == np.uint8 and got.shape == img.shape
        np.testing.assert_array_equal(got, g[key + "davis_a0.5"])
        np.testing.assert_array_equal(utils_ipn.overlay_fade(img, lab), g[key + "fade"])
        np.testing.assert_array_equal(utils_ipn.overlay_checker(img, lab.astype(np.int64)), g[key + "checker"])
        np.testing.assert_array_equal(utils_ipn.overlay_color(img, lab), g[key + "color"])
        np.testing.assert_array_equal(utils_ipn.overlay_color(img, lab, rgb=[3, 250, 9]), g[key + "color_rgb"])
        np.testing.assert_array_equal(img, keep)


# ================================================================================================ overlay_session
def test_overlay_session_on_both_frame_kinds_and_mask_types(dev):
    from ivos_w_amd.models.assessment import LabelMasks, PackedFrames
    n, H, W = 4, 17, 64
    img, lab = images(n, H, W), label_maps(n, H, W, 3)
    rgbx = torch.from_numpy(np.concatenate([img, np.zeros((n, H, W, 1), np.uint8)], 3)).to(dev)
    planes, lab_t = torch.from_numpy(planes_of(img)).to(dev), torch.from_numpy(lab).to(dev)
    for style in R.STYLES:
        want = R.overlay(img, lab, style, 3, frame_ids=[3, 1, 1], alpha=0.3)
        for frames in (PackedFrames(rgbx), planes):
            for labels in (lab_t, LabelMasks(lab_t)):
                got = utils_ipn.overlay_session(frames, labels, 3, style=style, frame_ids=[3, 1, 1], alpha=0.3)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W, 3)
                np.testing.assert_array_equal(got.cpu().numpy(), want)
    got = utils_ipn.overlay_session(PackedFrames(rgbx), lab_t, 3, out="rgbx", select=2, palette=[(1, 2, 3), (40, 50, 60)])
    np.testing.assert_array_equal(got.cpu().numpy(), R.overlay(img, lab, "davis", 3, out="rgbx", select=2, palette=[(1, 2, 3), (40, 50, 60), (0, 0, 0)]))
    strided = torch.from_numpy(np.repeat(lab, 2, axis=0)).to(dev)[::2]                        # a LabelMasks whose frames are strided
    np.testing.assert_array_equal(utils_ipn.overlay_session(planes, LabelMasks(strided), 3).cpu().numpy(), R.overlay(img, lab, "davis", 3))
    for bad in (dict(style="glow"), dict(out="bgr"), dict(frame_ids=[]), dict(frame_ids=[n]), dict(select=4), dict(alpha=1.5), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            utils_ipn.overlay_session(planes, lab_t, 3, **bad)
    with pytest.raises(TypeError):
        utils_ipn.overlay_session(planes, lab_t.float(), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils_ipn.overlay_session(planes.cpu(), lab_t.cpu(), 3)


def test_the_call_is_asynchronous_and_capture_safe(dev):
    """Recorded into a HIP graph, the call launches kernels only (no allocation, no copy, no synchronisation would survive a capture):
    nothing is written until the graph runs, and every replay draws the labels as they are then.  This drives the C entry: a capture
    forbids the torch.empty of overlay_session, whose "no synchronisation" holds by construction - one allocation and this one call."""
    n, H, W = 3, 9, 32
    img, lab = images(n, H, W), label_maps(n, H, W, 3)
    fb = Buf(dev, np.concatenate([img, np.zeros((n, H, W, 1), np.uint8)], 3), 1)
    lb, ob = Buf(dev, lab, 1), Buf(dev, np.full(2 * H * W * 3, OUT_FILL, np.uint8), OUT_FILL)
    opt, ids = options("davis", 3), L.int_array([2, 0])
    torch.cuda.synchronize(dev)
    with L.Graph.capture(dev) as g:
        L.check(L.lib().ivosw_overlay_frames(fb.ptr(), L.FRAMES_RGBX8, lb.ptr(), n, H, W, ids, 2, ctypes.byref(opt), ob.ptr(), L.OUT_RGB8,
                                             L.stream_ptr(dev)), "overlay_frames")
    assert g.kernel_nodes == 1, g.kernel_nodes
    torch.cuda.synchronize(dev)
    ob.back("out before the launch", unchanged=True)
    for labels in (lab, np.roll(lab, 1, axis=0)):
        lb.t[lb.lo:lb.lo + lb.n] = torch.from_numpy(labels.reshape(-1)).to(dev)
        g.launch()
        torch.cuda.synchronize(dev)
        np.testing.assert_array_equal(ob.back("out").reshape(2, H, W, 3), R.overlay(img, labels, "davis", 3, frame_ids=[2, 0]))


# ================================================================================================ refusals
def test_refusals_write_nothing(dev):
    n, H, W = 3, 9, 32
    img, lab = images(n, H, W), label_maps(n, H, W, 3)

    def opt_with(**fields):
        o = options("davis", 3)
        for k, v in fields.items():
            setattr(o, k, v)
        return ctypes.byref(o), o

    cases = [
        ("null frames", dict(frames=None), "null frames"), ("null labels", dict(labels=None), "null labels"),
        ("null out", dict(out=None), "null out"), ("null opt", dict(opt=None), "null opt"),
        ("frame kind", dict(frames_kind=2), "frames_kind"), ("frame kind -1", dict(frames_kind=-1), "frames_kind"),
        ("out kind", dict(out_kind=2), "out_kind"), ("style 4", dict(opt=opt_with(style=4)), "style"), ("style -1", dict(opt=opt_with(style=-1)), "style"),
        ("n_frames 0", dict(n_frames=0), "shape"), ("H 0", dict(H=0), "shape"), ("W -1", dict(W=-1), "shape"),
        ("H * W", dict(H=1 << 16, W=1 << 15), "INT_MAX"),
        ("n_objects 0", dict(opt=opt_with(n_objects=0, select=0)), "n_objects"), ("n_objects 33", dict(opt=opt_with(n_objects=33)), "n_objects"),
        ("select -1", dict(opt=opt_with(select=-1)), "select"), ("select 4", dict(opt=opt_with(select=4)), "select"),
        ("alpha < 0", dict(opt=opt_with(alpha=-1e-9)), "alpha"), ("alpha > 1", dict(opt=opt_with(alpha=1.0000001)), "alpha"),
        ("alpha nan", dict(opt=opt_with(alpha=float("nan"))), "alpha"),
        ("id n", dict(ids=L.int_array([0, 1, n]), n_ids=3), "frame_ids[2]"), ("id -1", dict(ids=L.int_array([-1, 1]), n_ids=2), "frame_ids[0]"),
        ("empty list", dict(ids=L.int_array([0]), n_ids=0), "length"), ("negative list", dict(ids=L.int_array([0]), n_ids=-3), "length"),
    ]
    for name, geom, word in cases:
        held = geom.get("opt")
        if isinstance(held, tuple):
            geom = dict(geom, opt=held[0])
        rc, _, _ = render(dev, img, lab, options("davis", 3), "rgbx", "rgbx", geom=geom)
        msg = L.lib().ivosw_last_error().decode()
        assert rc == -1 and "ivosw_overlay_frames" in msg and word in msg, (name, rc, msg)
    # misaligned RGBX8 pointers (frames, out), and an output that overlaps an input
    for kind, out, which in (("rgbx", "rgb", "frames"), ("rgbx", "rgbx", "out")):
        n_, H_, W_ = lab.shape
        for shift in (1, 2, 3):
            fb = Buf(dev, np.zeros(n_ * H_ * W_ * 4 + 8, np.uint8), 7)
            lb, ob = Buf(dev, lab, 1), Buf(dev, np.full(n_ * H_ * W_ * 4 + 8, OUT_FILL, np.uint8), OUT_FILL)
            p = lambda b, s: ctypes.c_void_p(b.ptr().value + s)
            o = options("fade", 3)
            rc = L.lib().ivosw_overlay_frames(p(fb, shift if which == "frames" else 0), L.FRAMES_RGBX8, lb.ptr(), n_, H_, W_, None, 0, ctypes.byref(o),
                                              p(ob, shift if which == "out" else 0), OUTS[out], L.stream_ptr(dev))
            torch.cuda.synchronize(dev)
            assert rc == -1 and "aligned" in L.lib().ivosw_last_error().decode(), (which, shift)
            for b in (fb, lb, ob):
                b.back(which, unchanged=True)
    fb = Buf(dev, np.concatenate([img, np.zeros((n, H, W, 1), np.uint8)], 3), 1)
    lb = Buf(dev, lab, 1)
    o = options("color", 3)
    last_px = n * H * W - 1
    for frames_ptr, out_ptr, ids, word in (
            (fb.ptr(), fb.ptr(), None, "overlaps frames"),
            (fb.ptr(), ctypes.c_void_p(fb.ptr().value + 4 * last_px), [0], "overlaps frames"),              # the last pixel of the frames
            (fb.ptr(), ctypes.c_void_p(fb.ptr().value - 4 * H * W + 4), [0], "overlaps frames"),            # ... and the first
            (fb.ptr(), lb.ptr(), [1], "overlaps labels"),
            (fb.ptr(), ctypes.c_void_p(lb.ptr().value + last_px - last_px % 4), [1], "overlaps labels")):
        rc = L.lib().ivosw_overlay_frames(frames_ptr, L.FRAMES_RGBX8, lb.ptr(), n, H, W, None if ids is None else L.int_array(ids),
                                          0 if ids is None else len(ids), ctypes.byref(o), out_ptr, L.OUT_RGBX8, L.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        assert rc == -1 and word in L.lib().ivosw_last_error().decode(), (word, L.lib().ivosw_last_error())
        fb.back("frames", unchanged=True)
        lb.back("labels", unchanged=True)
    # the neighbours of a refusal are accepted: alpha 0 and 1, select = n_objects, n_objects = 32, a list of one
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(select=3)):
        check(dev, img, lab, "davis", 3, **kw)
    check(dev, img, lab, "davis", 32, ids=[n - 1])


# ================================================================================================ a fresh process on the scalar kernels
CHILD = (2, 17, 64, 3)


def child_main(path):
    """Runs in the child process of the test below (IVOSW_OVERLAY_SCALAR=1 in its environment from the start)."""
    assert os.environ.get("IVOSW_OVERLAY_SCALAR") == "1"
    dev = torch.device("cuda:0")
    n, H, W, n_objects = CHILD
    img, lab = images(n, H, W), label_maps(n, H, W, n_objects)
    out = {}
    for style in R.STYLES:
        for kind, o in (("rgbx", "rgb"), ("f32", "rgbx")):
            rc, got, _ = render(dev, img, lab, options(style, n_objects, alpha=0.3), kind, o)
            assert rc == 0
            out[f"{style}_{kind}"] = got
    np.savez(path, **out)


def test_scalar_kernels_in_a_fresh_process(dev, tmp_path):
    path = str(tmp_path / "scalar.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, IVOSW_OVERLAY_SCALAR="1")
    r = subprocess.run([sys.executable, "-c", f"from tests import test_gpu_overlay as t; t.child_main({path!r})"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sca = np.load(path)
    n, H, W, n_objects = CHILD
    img, lab = images(n, H, W), label_maps(n, H, W, n_objects)
    for style in R.STYLES:
        for kind, o in (("rgbx", "rgb"), ("f32", "rgbx")):
            vec = check(dev, img, lab, style, n_objects, kind, o, alpha=0.3, why="vector")
            np.testing.assert_array_equal(sca[f"{style}_{kind}"], vec, err_msg=f"child: {style} {kind}")


# ================================================================================================ the entry point
def _read_picture(path):
    if path.endswith(".png"):
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"))
    with open(path, "rb") as fp:
        magic, dims, top = fp.readline(), fp.readline(), fp.readline()
        assert magic == b"P6\n" and top == b"255\n"
        w, h = (int(v) for v in dims.split())
        return np.frombuffer(fp.read(), np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("frames", ["uint8", "float32"])
def test_run_eval_writes_the_candidates_with_the_masks_drawn(dev, tmp_path, monkeypatch, capsys, frames):
    from ivos_w_amd import entry
    from ivos_w_amd.models.assessment import PackedFrames
    from ivos_w_amd.utils import utils_agent
    common = ["with", "synthetic=1", "setting=oracle", "method=ours", "synth.n_sequences=2", "synth.n_frames=8", "synth.height=48",
              "synth.width=80", "eval_max_nb_interactions=3", "agent.candidates=2", f"frames={frames}", f"ckpt_dir={tmp_path}/weights"]
    seen = []
    real = entry.write_overlays

    def spy(overlay, report_dir, sequence, visit, interaction, all_F, labels, n_objects, candidates, device):
        paths = real(overlay, report_dir, sequence, visit, interaction, all_F, labels, n_objects, candidates, device)
        seen.append(dict(paths=paths, sequence=sequence, visit=visit, interaction=interaction, all_F=all_F, labels=labels.cpu().numpy().copy(),
                         n_objects=n_objects, candidates=[int(c) for c in candidates]))
        return paths
    monkeypatch.setattr(entry, "write_overlays", spy)
    utils_agent.clear_frame_cache()
    out = entry.run_eval(entry.parse_cli(common + ["overlay=davis", "overlay_frames=candidates", f"report_save_dir={tmp_path}/drawn"]), "MANet")
    text = capsys.readouterr().out
    assert len(seen) == 2 * 3 and text.count("[ivos-w] overlay=davis: ") == 6
    root = os.path.join(out["report_dir"], "overlays")
    n_files = 0
    for s in seen:
        ids = sorted(set(s["candidates"]))
        ext = os.path.splitext(s["paths"][0])[1]
        assert s["paths"] == [os.path.join(root, f"{s['sequence']}_{s['visit']}", str(s["interaction"]), f"{f:05d}{ext}") for f in ids]
        if isinstance(s["all_F"], PackedFrames):
            img = s["all_F"].rgbx[..., :3].cpu().numpy()
        else:
            img = R.frame_bytes(s["all_F"].cpu().numpy())                # the byte rule on the frames the session used
        assert (frames == "uint8") == isinstance(s["all_F"], PackedFrames)
        want = R.overlay(img, s["labels"], "davis", s["n_objects"], frame_ids=ids)
        for j, p in enumerate(s["paths"]):
            np.testing.assert_array_equal(_read_picture(p), want[j], err_msg=p)
            n_files += 1
        assert f"overlay=davis: {len(ids)} pictures of {s['sequence']}_{s['visit']}, interaction {s['interaction']}," in text
    assert n_files == sum(len(fs) for _, _, fs in os.walk(root)) >= 6
    # overlay=none: no directory, and the summary is byte for byte that of a run without the key
    summaries = []
    for name, extra, drop in (("none", ["overlay=none"], False), ("absent", [], True)):
        cfg = entry.parse_cli(common + extra + [f"report_save_dir={tmp_path}/{name}"])
        if drop:
            del cfg["overlay"], cfg["overlay_frames"]
        calls = len(seen)
        utils_agent.clear_frame_cache()
        o = entry.run_eval(cfg, "MANet")
        assert len(seen) == calls and not os.path.exists(os.path.join(o["report_dir"], "overlays"))
        summaries.append(open(os.path.join(o["report_dir"], "summary.json"), "rb").read())
    assert summaries[0] == summaries[1] == open(os.path.join(out["report_dir"], "summary.json"), "rb").read()
    assert "overlay=" not in capsys.readouterr().out
    json.loads(summaries[0])


def test_run_eval_overlay_frames_all(dev, tmp_path, capsys):
    from ivos_w_amd import entry
    cfg = entry.parse_cli(["with", "synthetic=1", "setting=oracle", "method=ours", "synth.n_sequences=1", "synth.n_frames=6", "synth.height=24",
                           "synth.width=36", "eval_max_nb_interactions=2", "overlay=checker", "overlay_frames=all", f"ckpt_dir={tmp_path}/weights",
                           f"report_save_dir={tmp_path}/all"])
    out = entry.run_eval(cfg, "MANet")
    root = os.path.join(out["report_dir"], "overlays")
    files = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    assert len(files) == 2 * 6 and [os.path.basename(f)[:5] for f in files[:6]] == [f"{f:05d}" for f in range(6)]
    assert capsys.readouterr().out.count("overlay=checker: 6 pictures") == 2
