"""8-bit video frames in the assessment path, without a GPU: the C ABI and its binding declare the four _u8 entries, the host types
(PackedFrames, AssessNet.pack_frames, utils_agent.pack_video) exist and refuse what they must before anything touches a device, the
entry points carry ``frames=float32|uint8``, a numpy mirror of the packing gives the bytes written by hand for a 2x3 image, and the
byte -> colour conversion is pinned: the two host conventions agree on all 256 values, and so does the sampler's division by 255."""
import ctypes
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_and_binding_declare_the_entries():
    S = L.SIGNATURES
    assert S["ivosw_frames_pack_u8"] == (L._i, [L._p, L._i, L._i, L._i, L._i, L._p, L._p])
    assert S["ivosw_roi_sample_u8"] == S["ivosw_roi_sample"]                        # rgbx in place of tf, nothing else
    assert S["ivosw_assess_forward_u8"] == S["ivosw_assess_forward"]
    assert S["ivosw_assess_forward_objects_u8"] == S["ivosw_assess_forward_objects"]
    assert (L.U8_HWC3, L.U8_CHW3) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for name in ("int ivosw_frames_pack_u8(const uint8_t* src, int layout, int n, int H, int W, uint8_t* rgbx, ivosw_stream_t stream)",
                 "int ivosw_roi_sample_u8(const uint8_t* rgbx, const float* tp, const float* yxhw, int B, int H, int W,",
                 "int ivosw_assess_forward_u8(const void* packed, int dtype, const uint8_t* rgbx, const float* tp,",
                 "int ivosw_assess_forward_objects_u8(const void* packed, int dtype, const uint8_t* rgbx, int n_frames, const float* masks,",
                 "IVOSW_U8_HWC3 0", "IVOSW_U8_CHW3 1"):
        assert name in hdr, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ivosw_frames_pack_u8", "ivosw_roi_sample_u8", "ivosw_assess_forward_u8", "ivosw_assess_forward_objects_u8", "PackedFrames"):
        assert name in doc, name


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _fake(offset=0):
    """A non-NULL host pointer that must never be dereferenced: every case below is refused before any pointer is used."""
    buf = ctypes.create_string_buffer(96)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, ctypes.c_void_p(base + offset)


def _msg(lib):
    return lib.ivosw_last_error().decode()


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    keep, p = _fake()
    keep1, odd = _fake(1)
    keep2, half = _fake(2)
    # pack: NULL, layout, sizes, a misaligned destination; a source of any alignment is taken (it reaches the device-pointer check)
    assert lib.ivosw_frames_pack_u8(None, 0, 1, 4, 4, p, None) == -1 and "null pointer" in _msg(lib)
    assert lib.ivosw_frames_pack_u8(p, 0, 1, 4, 4, None, None) == -1 and "null pointer" in _msg(lib)
    for layout in (-1, 2, 7):
        assert lib.ivosw_frames_pack_u8(p, layout, 1, 4, 4, p, None) == -1 and "layout" in _msg(lib), layout
    for n, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib.ivosw_frames_pack_u8(p, 0, n, H, W, p, None) == -1 and "must be positive" in _msg(lib)
    assert lib.ivosw_frames_pack_u8(p, 0, 1, 65536, 65536, p, None) == -1 and "too large" in _msg(lib)
    for bad in (odd, half):
        assert lib.ivosw_frames_pack_u8(p, 1, 1, 4, 4, bad, None) == -1 and "4-byte aligned" in _msg(lib)
    assert lib.ivosw_frames_pack_u8(odd, 0, 1, 1, 1, p, None) == -1 and "not a device pointer" in _msg(lib)    # H, W >= 1 is enough here
    assert "ivosw_frames_pack_u8" in _msg(lib)
    # sampler
    assert lib.ivosw_roi_sample_u8(None, p, p, 1, 4, 4, 0, p, None) == -1 and "null pointer" in _msg(lib)
    assert lib.ivosw_roi_sample_u8(odd, p, p, 1, 4, 4, 0, p, None) == -1 and "4-byte aligned" in _msg(lib)
    assert lib.ivosw_roi_sample_u8(p, p, p, 1, 1, 4, 0, p, None) == -1 and "H, W > 1" in _msg(lib)
    assert lib.ivosw_roi_sample_u8(p, p, p, 1, 4, 4, 9, p, None) == -1 and "dtype" in _msg(lib)
    assert lib.ivosw_roi_sample_u8(p, p, p, 1, 4, 4, 0, p, None) == -1 and "not a device pointer" in _msg(lib)
    # the forward entries: the fp32 entries' refusals (their size checks come behind the device lookup, as ever) plus the alignment
    fwd = lambda rgbx, H=8, W=8, B=1: lib.ivosw_assess_forward_u8(p, 1, rgbx, p, B, H, W, p, p, 1 << 20, 0, 0, None, None)
    assert fwd(None) == -1 and "null pointer" in _msg(lib)
    assert fwd(half) == -1 and "4-byte aligned" in _msg(lib)
    assert fwd(p) == -1 and "not a device pointer" in _msg(lib)
    obj = lambda rgbx, n=2, o=2: lib.ivosw_assess_forward_objects_u8(p, 1, rgbx, n, p, 64, 64, o, 8, 8, p, p, 1 << 20, 0, None)
    assert obj(None) == -1 and "null pointer" in _msg(lib)
    assert obj(odd) == -1 and "4-byte aligned" in _msg(lib)
    assert obj(p, n=0) == -1 and "must be positive" in _msg(lib)
    assert obj(p) == -1 and "not a device pointer" in _msg(lib)
    # the fp32 entries take a float pointer of any 4-byte alignment as before: no new refusal on their side
    assert lib.ivosw_assess_forward(p, 1, p, p, 1, 8, 8, p, p, 1 << 20, 0, 0, None, None) == -1 and "not a device pointer" in _msg(lib)


def test_version_is_unchanged(lib):
    assert lib.ivosw_version() == 102


def test_new_kernels_have_no_scratch_and_the_float_sampler_is_still_there(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    table = kr.kernel_table(L.LIB_PATH)
    pick = lambda key: [r for n, r in table.items() if key in n]
    for key, count in (("roi_sample_u8_kernel", 2), ("frames_pack_u8_kernel", 1), ("roi_sample_kernel", 2)):
        hits = pick(key)
        assert len(hits) == count, (key, hits)
        assert all(r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 for r in hits), (key, hits)
    # the 8-bit sampler holds pixel words where the float one holds 12 colour floats per row pair: never more registers
    old = {n.split("roi_sample_kernel")[1][:3]: r for n, r in table.items() if "roi_sample_kernel" in n}
    new = {n.split("roi_sample_u8_kernel")[1][:3]: r for n, r in table.items() if "roi_sample_u8_kernel" in n}
    assert sorted(old) == sorted(new) and all(new[k]["vgpr"] <= old[k]["vgpr"] for k in old), (old, new)


# ---------------------------------------------------------------------------------------------- host types
def test_packed_frames_and_the_packers_refuse_bad_input():
    from ivos_w_amd.models.assessment import AssessNet, PackedFrames, pack_frames
    from ivos_w_amd.utils import utils_agent
    net = AssessNet()
    ok = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    for pack in (net.pack_frames, lambda u8, **k: utils_agent.pack_video(u8, "cpu", **k), lambda u8, **k: pack_frames(u8, "cpu", **k)):
        for bad in (ok.float(), ok.to(torch.int8), ok.to(torch.int16), ok.numpy().astype(np.uint16), ok.numpy().astype(np.float32),
                    [[1, 2, 3]], None):
            with pytest.raises(TypeError, match="uint8"):
                pack(bad)
        for bad, kw in ((ok, dict(layout="chw")), (ok.permute(0, 3, 1, 2), {}), (ok[0], {}), (ok[..., :2], {}),
                        (torch.zeros(0, 5, 7, 3, dtype=torch.uint8), {}), (torch.zeros(2, 3, 5, 7, 1, dtype=torch.uint8), dict(layout="chw")),
                        (np.zeros((2, 4, 5, 7), np.uint8), dict(layout="chw"))):
            with pytest.raises(ValueError, match="layout"):
                pack(bad, **kw)
        for layout in ("HWC", "nhwc", "", None, 0):
            with pytest.raises(ValueError, match="layout"):
                pack(ok, layout=layout)
        # a 3x3-pixel video fits both layouts: the argument decides, "hwc" by default; with valid input the packer reaches the device
        # and there is no CPU fallback
        amb = torch.zeros(3, 3, 3, 3, dtype=torch.uint8)
        for kw in ({}, dict(layout="hwc"), dict(layout="chw")):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                pack(amb, **kw)
    with pytest.raises(TypeError):
        PackedFrames(torch.zeros(2, 5, 7, 4))
    with pytest.raises(TypeError):
        PackedFrames(np.zeros((2, 5, 7, 4), np.uint8))
    for shape in ((2, 5, 7, 3), (5, 7, 4), (2, 4, 5, 7)):
        with pytest.raises(ValueError):
            PackedFrames(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        PackedFrames(torch.zeros(2, 5, 7, 8, dtype=torch.uint8)[..., ::2])            # not contiguous
    pf = PackedFrames(torch.arange(2 * 5 * 7 * 4, dtype=torch.int32).to(torch.uint8).view(2, 5, 7, 4))
    assert (pf.n, pf.H, pf.W, len(pf)) == (2, 5, 7, 2) and pf.device == torch.device("cpu")
    f = pf.to_float()
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 3, 5, 7) and f.is_contiguous()
    assert torch.equal(f, pf.rgbx[..., :3].permute(0, 3, 1, 2).float() / 255.)
    # the frame cache hands a PackedFrames on as it is: no upload, no copy
    cache = utils_agent._FrameCache()
    assert cache.get(pf, "cpu") is pf and cache.uploads == 0 and cache.frames is None


def test_forward_reaches_the_u8_entry_only_through_packed_frames(monkeypatch):
    """The dispatch, with the library replaced: a PackedFrames goes to the _u8 entries with its own B, H, W, checked against the masks; a
    plain uint8 tensor is cast to float32 WITHOUT scaling and goes to the float entries, as it always did."""
    from ivos_w_amd.models import assessment as A
    calls = []

    class FakeLib:
        def ivosw_assess_ws_bytes(self, *a):
            return 16

        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, a))
                return 0
            return fn

    monkeypatch.setattr(A.L, "lib", lambda: FakeLib())
    monkeypatch.setattr(A.L, "dptr", lambda t, dtype=None: t)
    monkeypatch.setattr(A.L, "stream_ptr", lambda dev=None: None)
    net = A.AssessNet(precision="bf16").eval()
    monkeypatch.setattr(net, "_ensure_packed", lambda: torch.zeros(1))
    pf = A.PackedFrames(torch.full((2, 6, 8, 4), 255, dtype=torch.uint8))
    tp = torch.zeros(2, 6, 8)
    net(pf, tp)
    name, a = calls[-1]
    assert name == "ivosw_assess_forward_u8" and a[2] is pf.rgbx and a[4:7] == (2, 6, 8)
    net.forward_tap(pf, tp, "roi")
    assert calls[-1][0] == "ivosw_assess_forward_u8" and calls[-1][1][11] == 1
    net.forward_objects(pf, torch.zeros(2, 3, 6, 8), 2)
    name, a = calls[-1]
    assert name == "ivosw_assess_forward_objects_u8" and a[2] is pf.rgbx and a[3] == 2 and a[7:10] == (2, 6, 8)
    for bad_tp in (torch.zeros(3, 6, 8), torch.zeros(2, 8, 6)):
        with pytest.raises(AssertionError):
            net(pf, bad_tp)
    with pytest.raises(AssertionError):
        net.forward_objects(pf, torch.zeros(3, 3, 6, 8), 2)
    u8 = torch.full((2, 3, 6, 8), 255, dtype=torch.uint8)
    net(u8, tp)
    name, a = calls[-1]
    assert name == "ivosw_assess_forward" and a[2].dtype == torch.float32 and float(a[2].max()) == 255.0       # unscaled
    net.forward_objects(u8, torch.zeros(2, 3, 6, 8), 2)
    assert calls[-1][0] == "ivosw_assess_forward_objects" and float(calls[-1][1][2].max()) == 255.0


# ---------------------------------------------------------------------------------------------- entry points
def test_cli_carries_the_frames_option(tmp_path):
    assert entry.DEFAULTS["frames"] == "float32"
    assert entry.parse_cli([]).frames == "float32"
    assert entry.parse_cli(["with", "frames=uint8"]).frames == "uint8"
    assert entry.parse_cli(["with", "frames=float32"]).frames == "float32"
    y = tmp_path / "c.yaml"
    y.write_text("frames: uint8\n")
    assert entry.parse_cli(["--config", str(y)]).frames == "uint8"
    for bad in ("uint16", "u8", "UINT8", "float16", "8", "true", "none", ""):
        with pytest.raises(SystemExit, match="frames"):
            entry.parse_cli(["with", f"frames={bad}"])
    with pytest.raises(SystemExit, match="frames"):
        entry.parse_cli([], frames=8)
    # read with .get: a config written before the key existed keeps the float frames; run_eval refuses a bad value before any work
    assert entry.frames_option({}) == "float32" and entry.frames_option(dict(frames="uint8")) == "uint8"
    cfg = entry.parse_cli(["with", "synthetic=1"])
    cfg.frames = "uint16"
    with pytest.raises(ValueError, match="frames"):
        entry.run_eval(cfg)
    with pytest.raises(ValueError, match="frames"):
        entry.SyntheticDavis(cfg, torch.device("cpu"))
    cfg.frames = "float32"
    dv = entry.SyntheticDavis(entry.parse_cli(["with", "synth.n_frames=4", "synth.height=16", "synth.width=24"]), torch.device("cpu"))
    f = dv.load_frames("synth-00")
    assert f.dtype == torch.float32 and tuple(f.shape) == (4, 3, 16, 24)            # float32 mode: what it always returned


# ---------------------------------------------------------------------------------------------- the packing and the conversion
def pack_mirror(u8, layout):
    """numpy mirror of ivosw_frames_pack_u8: [n,H,W,3] ("hwc") or [n,3,H,W] ("chw") -> RGBX8 [n,H,W,4] with X = 0."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and layout in ("hwc", "chw")
    hwc = u8 if layout == "hwc" else u8.transpose(0, 2, 3, 1)
    out = np.zeros(hwc.shape[:3] + (4,), np.uint8)
    out[..., :3] = hwc
    return out


def test_pack_mirror_matches_hand_written_bytes():
    # one 2x3 image: pixel (y, x) has R = 10 y + x, G = 100 + R, B = 200 + R
    want = bytes([0, 100, 200, 0, 1, 101, 201, 0, 2, 102, 202, 0,
                  10, 110, 210, 0, 11, 111, 211, 0, 12, 112, 212, 0])
    hwc = np.array([[[[0, 100, 200], [1, 101, 201], [2, 102, 202]],
                     [[10, 110, 210], [11, 111, 211], [12, 112, 212]]]], np.uint8)
    chw = np.array([[[[0, 1, 2], [10, 11, 12]],
                     [[100, 101, 102], [110, 111, 112]],
                     [[200, 201, 202], [210, 211, 212]]]], np.uint8)
    assert hwc.shape == (1, 2, 3, 3) and chw.shape == (1, 3, 2, 3)
    assert pack_mirror(hwc, "hwc").tobytes() == want
    assert pack_mirror(chw, "chw").tobytes() == want
    # as 32-bit words (what the sampler loads): R | G << 8 | B << 16, little endian
    words = np.frombuffer(want, "<u4")
    assert [int(w) for w in words[:2]] == [0 | 100 << 8 | 200 << 16, 1 | 101 << 8 | 201 << 16]


def test_both_host_conventions_give_the_same_256_colours():
    a = np.arange(256, dtype=np.float32) / 255.
    b = (np.arange(256) / 255.).astype(np.float32)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    c = (torch.arange(256, dtype=torch.uint8).float() / 255.).numpy()
    assert np.array_equal(a.view(np.int32), c.view(np.int32))
    assert a[0] == 0.0 and a[255] == 1.0


def _rn32(x):
    """A positive Fraction rounded to the nearest float32 (ties to even), as a Fraction; normal range only."""
    if x == 0:
        return Fraction(0)
    sign, a = (1, x) if x > 0 else (-1, -x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    assert e >= -126
    ulp = Fraction(2) ** (e - 23)
    q = a / ulp
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return sign * f * ulp


def test_the_samplers_division_by_255_is_correctly_rounded_for_every_byte():
    """The device converts a byte with q = v * r, e = fma(-q, 255, v), q + e * r (r = float32(1 / 255)): a reciprocal product and one
    Newton step on the residual.  In exact rational arithmetic, with one rounding per operation as the hardware does, it equals the
    correctly rounded float32(v) / float32(255) for all 256 bytes; the plain product v * r alone does not."""
    r = Fraction(float(np.float32(1.0) / np.float32(255.0)))
    assert _rn32(Fraction(1, 255)) == r
    want = np.arange(256, dtype=np.float32) / np.float32(255.0)
    plain_wrong = 0
    for v in range(256):
        q = _rn32(v * r)
        e = _rn32(v - q * 255)                      # one fma: a single rounding of the exact value
        got = _rn32(q + e * r)
        assert _rn32(Fraction(v, 255)) == Fraction(float(want[v])), v          # numpy's division is the correctly rounded one
        assert got == Fraction(float(want[v])), v
        plain_wrong += q != Fraction(float(want[v]))
    assert plain_wrong > 0
