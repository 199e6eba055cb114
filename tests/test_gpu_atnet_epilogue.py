"""GPU: the ATNet epilogue (csrc/atnet_epilogue.hip) through the C ABI on a case table that runs its three kernels (vector loads with
vector window stores, vector loads with element window stores, scalar).

The sigmoid - read from prob_pad, the unblended output - against the float64 sigmoid of tests/atnet_ref.py:

    err_kernel <= SIG_MULT * err_torch + SIG_FLOOR

err_torch is the error of torch.sigmoid on the CPU in float32 on the same logits against the same float64 values, both as largest
absolute errors over a case (the scheme of tests/test_gpu_seg_edges.py).  SIG_FLOOR = 2^-24 is half an ulp of a probability in
[0.5, 1).  SIG_MULT = 2 was set after the first run on an MI355X to the next integer above the largest measured ratio (LAB_NOTES.md,
"ATNet epilogue against float64", has both errors and the ratio for every case).  Terms whose float64 value is below float32's smallest
normal number are held to an absolute bound only (0 <= s <= 2^-125); sigmoid(0) is 0.5 bit for bit.

Everything behind the sigmoid is exact and asserted bit for bit, recomputed on the host from the kernel's own prob_pad: the map in
place (three separately rounded float32 operations, or s itself), the store slot (the crop of the map), the labels (first maximum,
strictly above th).  Every buffer lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from tests import atnet_ref as ar

pytestmark = pytest.mark.gpu

SIG_MULT, SIG_FLOOR = ar.SIG_MULT, ar.SIG_FLOOR
PAD = 16                    # elements in front of and behind every buffer: a multiple of 16 bytes for each type
N_FRAMES = 3
FILL = {"logits": 0.25, "map": -3.0, "pad": -7.0, "probs": -7.0, "u8": 77, "f32": -7.0}
OUTS = ("pad", "probs", "u8", "f32")
ALPHAS = (None, 1, 0.5, 0.75, 0.5 + 0.5 / 3)          # None: blend = 0

Case = namedtuple("Case", "name n_obj PH PW pads wide")
CASES = [Case("vec", 3, 20, 36, (2, 2, 4, 4), False), Case("shift", 3, 20, 36, (1, 3, 3, 5), False), Case("odd", 2, 9, 37, (1, 1, 3, 2), False),
         Case("one", 1, 8, 12, (1, 1, 4, 4), False), Case("max", 255, 6, 8, (1, 1, 2, 2), False), Case("wide", 3, 20, 36, (2, 2, 4, 4), True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _vector_path_unless_asked(monkeypatch):
    monkeypatch.delenv("IVOSW_ATNET_SCALAR", raising=False)


def _hw(c):
    return c.PH - c.pads[0] - c.pads[1], c.PW - c.pads[2] - c.pads[3]


_DATA = {}


def _data(c):
    """(logits [n_obj,PH,PW], map [3,n_obj,PH,PW]) of a case, seeded; made once and never written."""
    if c.name not in _DATA:
        rng = np.random.default_rng(sum(map(ord, c.name)))
        x = (rng.standard_normal((c.n_obj, c.PH, c.PW)) * 3).astype(np.float32)
        if c.wide:                                        # saturation on both sides, results down to denormals and zero
            x[0] *= 20
            x[1] += 100
            x[2] -= 100
        x[0, 1, :2] = (0.0, -0.0)
        x[-1, 2, 5:7] = x[0, 2, 5:7]                      # two objects with equal logits
        m = rng.random((N_FRAMES, c.n_obj, c.PH, c.PW), dtype=np.float32)
        x.setflags(write=False)
        m.setflags(write=False)
        _DATA[c.name] = (x, m)
    return _DATA[c.name]


def _run(dev, c, x, m, t, alpha=None, th=0.5, want=OUTS, off=None, sc=None, n_obj=None, geom=None):
    """ivosw_atnet_epilogue on frame t -> (rc, {name: numpy}).  x None: logits = NULL.  Every buffer lies PAD elements inside an
    allocation of its own, moved by off[name] further elements (0: 16-byte aligned); the elements around it must keep their fill, and
    after a refused call every buffer must be what it was.  The map comes back whole ([3,n_obj,PH,PW]), the store whole
    ([n_obj+1,3,H,W], object-major, made at its fill: channel 0 must keep it)."""
    off = off or {}
    n_obj = n_obj or c.n_obj
    H, W = _hw(c)
    plane = c.PH * c.PW
    init = {"logits": None if x is None else np.ascontiguousarray(x).reshape(-1), "map": np.ascontiguousarray(m).reshape(-1),
            "pad": np.full(c.n_obj * plane, FILL["pad"], np.float32), "probs": np.full((c.n_obj + 1) * N_FRAMES * H * W, FILL["probs"], np.float32),
            "u8": np.full(H * W, FILL["u8"], np.uint8), "f32": np.full(H * W, FILL["f32"], np.float32)}
    first = {"logits": 0, "map": t * c.n_obj * plane, "pad": 0, "probs": (N_FRAMES + t) * H * W, "u8": 0, "f32": 0}
    bufs, ptrs, lo = {}, {}, {}
    for name in init:
        ptrs[name] = None
        if init[name] is None or (name in OUTS and name not in want):
            continue
        host = np.full(init[name].size + 3 * PAD, FILL[name], init[name].dtype)
        lo[name] = PAD + off.get(name, 0)
        host[lo[name]:lo[name] + init[name].size] = init[name]
        init[name] = host
        bufs[name] = torch.from_numpy(host).to(dev)
        assert bufs[name].data_ptr() % 16 == 0
        ptrs[name] = ctypes.c_void_p(bufs[name].data_ptr() + (lo[name] + first[name]) * bufs[name].element_size())
    g = dict(PH=c.PH, PW=c.PW, hpad1=c.pads[0], wpad1=c.pads[2], H=H, W=W, blend=int(alpha is not None))
    g.update(geom or {})
    a32, b32 = ar.alpha_beta32(1 if alpha is None else alpha)
    rc = L.lib().ivosw_atnet_epilogue(ptrs["logits"], ptrs["map"], n_obj, g["PH"], g["PW"], g["hpad1"], g["wpad1"], g["H"], g["W"], g["blend"],
                                      float(a32), float(b32), float(np.float32(th)), ptrs["pad"], ptrs["probs"],
                                      N_FRAMES * H * W if sc is None else sc, ptrs["u8"], ptrs["f32"], L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    shape = {"map": (N_FRAMES, c.n_obj, c.PH, c.PW), "pad": (c.n_obj, c.PH, c.PW), "probs": (c.n_obj + 1, N_FRAMES, H, W), "u8": (H, W), "f32": (H, W)}
    out = {}
    for name, buf in bufs.items():
        h = buf.cpu().numpy()
        a, b = lo[name], lo[name] + h.size - 3 * PAD
        assert (h[:a] == FILL[name]).all() and (h[b:] == FILL[name]).all(), f"{name}: written outside its extent"
        if rc != 0 or name == "logits":
            np.testing.assert_array_equal(h.view(np.uint8), init[name].view(np.uint8), err_msg=f"{name}: written by a refused call / an input")
        if name != "logits":
            out[name] = h[a:b].reshape(shape[name])
    return rc, out


def _assert_same_bits(a, b, why):
    for name in a:
        np.testing.assert_array_equal(a[name].view(np.uint8), b[name].view(np.uint8), err_msg=f"{why}: {name}")


def _check_behind_s(c, out, s, m, t, alpha, th):
    """Everything the kernel derives from s, bit for bit; s is the kernel's own prob_pad (or, without logits, nothing: p = the map)."""
    p = m[t] if s is None else (s if alpha is None else ar.blend32(s, m[t], alpha))
    want_map = m.copy()
    want_map[t] = p
    np.testing.assert_array_equal(out["map"].view(np.uint32), want_map.view(np.uint32), err_msg="map")
    win = ar.crop(p, c.pads)
    if "probs" in out:
        want = np.full_like(out["probs"], FILL["probs"])                      # channel 0 and the other frames' slots: untouched
        want[1:, t] = win
        np.testing.assert_array_equal(out["probs"].view(np.uint32), want.view(np.uint32), err_msg="store")
    lab = ar.labels(win, th)
    if "u8" in out:
        np.testing.assert_array_equal(out["u8"], lab)
    if "f32" in out:
        np.testing.assert_array_equal(out["f32"], lab.astype(np.float32))
    return p


def _check_sigmoid(name, s, x):
    ref = ar.sigmoid64(x)
    tiny = ref < ar.FLT_MIN
    s_t = torch.sigmoid(torch.from_numpy(np.array(x))).numpy()
    err_k = float(np.abs(s.astype(np.float64) - ref)[~tiny].max())
    err_t = float(np.abs(s_t.astype(np.float64) - ref)[~tiny].max())
    print(f"ATNETFIG {name} err_kernel={err_k:.3e} err_torch={err_t:.3e} ratio={err_k / err_t if err_t else float('nan'):.2f} tiny={int(tiny.sum())}")
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all()
    assert (s[tiny] <= 2.0 ** -125).all()
    assert (s[x == 0] == np.float32(0.5)).all() and (x == 0).sum() >= 2
    assert err_k <= SIG_MULT * err_t + SIG_FLOOR, (err_k, err_t)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_case_table(dev, monkeypatch, c):
    """blend = 0 and blend = 1 with every alpha, in the first and the last frame's slot; the scalar kernel and every one-element pointer
    offset give the same bits; each output alone gives what it gives with the others."""
    x, m = _data(c)
    th = 0.5
    for alpha in ALPHAS:
        for t in (0, N_FRAMES - 1):
            rc, out = _run(dev, c, x, m, t, alpha, th)
            assert rc == 0, L.lib().ivosw_last_error()
            if alpha is None and t == 0:
                _check_sigmoid(c.name, out["pad"], x)
            _check_behind_s(c, out, out["pad"], m, t, alpha, th)
            if alpha == 1:                                # 1 * s + 0 * old: the unblended result
                np.testing.assert_array_equal(out["map"][t].view(np.uint32), out["pad"].view(np.uint32))
            if t != 0 or alpha not in (None, 0.75):
                continue
            monkeypatch.setenv("IVOSW_ATNET_SCALAR", "1")                     # read by the launcher at every call
            rc, sca = _run(dev, c, x, m, t, alpha, th)
            monkeypatch.delenv("IVOSW_ATNET_SCALAR")
            assert rc == 0
            _assert_same_bits(out, sca, "IVOSW_ATNET_SCALAR")
            for off in ({"logits": 1}, {"map": 1}, {"pad": 1}, {"probs": 1}, {"u8": 1}, {"u8": 2}, {"f32": 1}, {"probs": 3, "u8": 3, "f32": 2, "map": 2}):
                rc, got = _run(dev, c, x, m, t, alpha, th, off=off)
                assert rc == 0
                _assert_same_bits(out, got, f"offset {off}")
            for one in OUTS + ((),):
                want = (one,) if one else ()                                  # (): the map alone
                rc, got = _run(dev, c, x, m, t, alpha, th, want=want)
                assert rc == 0
                _assert_same_bits({k: out[k] for k in got}, got, f"alone {want}")
                assert set(got) == set(want) | {"map"}


def test_the_label_limit(dev):
    """255 objects fit a uint8 label (the last object wins somewhere: label 255); 256 are refused when label_u8 is wanted and accepted
    with label_f32 only."""
    c = [c for c in CASES if c.name == "max"][0]
    x, m = _data(c)
    x = x.copy()
    x[254, 2, 3] = 50.0
    rc, out = _run(dev, c, x, m, 1)
    assert rc == 0 and out["u8"][1, 1] == 255 and out["f32"][1, 1] == 255.0
    c256 = c._replace(n_obj=256)
    x256 = np.concatenate([x, x[:1] + 60.0])
    m256 = np.concatenate([m, m[:, :1]], axis=1)
    rc, _ = _run(dev, c256, x256, m256, 1)
    assert rc == -1 and b"n_obj <= 255" in L.lib().ivosw_last_error()
    rc, out = _run(dev, c256, x256, m256, 1, want=("pad", "probs", "f32"))
    assert rc == 0
    _check_behind_s(c256, out, out["pad"], m256, 1, None, 0.5)
    assert out["f32"][1, 1] == 255.0 and (out["f32"] == 256.0).any()


def test_ties_and_the_threshold(dev):
    c = CASES[0]
    x, m = _data(c)
    x = x.copy()
    x[2] = x[1]                                           # objects 1 and 2 tie everywhere: never label 3
    rc, out = _run(dev, c, x, m, 0, th=0.0)
    assert rc == 0 and set(np.unique(out["u8"]).tolist()) <= {1, 2} and (out["u8"] == 2).any()
    x[0] = x[1]                                           # all three tie: the lowest index
    rc, out = _run(dev, c, x, m, 0, th=0.0)
    assert rc == 0 and (out["u8"] == 1).all() and (out["f32"] == 1.0).all()
    z = np.zeros_like(x)                                  # p == 0.5 everywhere: strictly above th or nothing
    rc, out = _run(dev, c, z, m, 0, th=0.5)
    assert rc == 0 and (out["pad"] == np.float32(0.5)).all() and (out["u8"] == 0).all() and (out["f32"] == 0.0).all()
    rc, out = _run(dev, c, z, m, 0, th=np.nextafter(np.float32(0.5), np.float32(0)))
    assert rc == 0 and (out["u8"] == 1).all() and (out["f32"] == 1.0).all()


@pytest.mark.parametrize("name", ["vec", "shift", "odd"])
def test_null_logits_rebuild_from_the_map(dev, monkeypatch, name):
    """logits = NULL: the labels and the slot come from an arbitrary finite map; the map keeps its bits; prob_pad is not written."""
    c = [c for c in CASES if c.name == name][0]
    _, m = _data(c)
    m = (m * 4 - 2).astype(np.float32)                    # any finite values, negative ones included
    for t in (0, 2):
        rc, out = _run(dev, c, None, m, t, th=0.25)
        assert rc == 0
        assert (out["pad"] == FILL["pad"]).all()
        _check_behind_s(c, out, None, m, t, None, 0.25)
        monkeypatch.setenv("IVOSW_ATNET_SCALAR", "1")
        rc, sca = _run(dev, c, None, m, t, th=0.25)
        monkeypatch.delenv("IVOSW_ATNET_SCALAR")
        assert rc == 0
        _assert_same_bits(out, sca, "scalar")
        rc, got = _run(dev, c, None, m, t, th=0.25, want=("u8",))
        assert rc == 0
        np.testing.assert_array_equal(got["u8"], out["u8"])


def test_refusals_write_nothing(dev):
    c = CASES[0]
    x, m = _data(c)
    H, W = _hw(c)
    err = lambda: L.lib().ivosw_last_error()
    for kw, text in ((dict(n_obj=-1), b"n_obj < 1"), (dict(geom=dict(H=0)), b"bad shape"), (dict(geom=dict(W=0)), b"bad shape"),
                     (dict(geom=dict(hpad1=-1)), b"negative pad"), (dict(geom=dict(wpad1=-1)), b"negative pad"),
                     (dict(geom=dict(hpad1=c.pads[0] + c.pads[1] + 1)), b"outside the padded grid"),
                     (dict(geom=dict(wpad1=c.pads[2] + c.pads[3] + 1)), b"outside the padded grid"), (dict(sc=H * W - 1), b"overlap"),
                     (dict(geom=dict(PH=1 << 16, PW=1 << 15)), b"too large"), (dict(geom=dict(PH=1 << 15, PW=1 << 15)), b"too large"),
                     (dict(geom=dict(blend=2)), b"0 or 1")):
        rc, _ = _run(dev, c, x, m, 1, **kw)               # (_run asserts that every buffer is what it was)
        assert rc == -1 and text in err(), (kw, err())
    rc, _ = _run(dev, c, None, m, 1, alpha=0.5)
    assert rc == -1 and b"blend needs logits" in err()
    rc, _ = _run(dev, c, None, m, 1, want=())
    assert rc == -1 and b"no output" in err()
    rc, _ = _run(dev, c, None, m, 1, want=("pad",))       # prob_pad is not an output without logits
    assert rc == -1 and b"no output" in err()
    rc = L.lib().ivosw_atnet_epilogue(None, None, 1, 4, 4, 1, 1, 2, 2, 0, 1.0, 0.0, 0.5, None, None, 0, None, None, L.stream_ptr(dev))
    assert rc == -1 and b"null prob_map_t" in err()
