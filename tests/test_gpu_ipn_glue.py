"""GPU: the two IPN glue kernels (csrc/ipn_glue.hip) through the C ABI against the numpy references of tests/ipn_ref.py, every
comparison bit for bit: nothing here is approximate - the dilation is integer work, the blend is three separately rounded float32
operations that numpy reproduces exactly, the labels are numpy's argmax.  (One allowance: where both the kernel and numpy hold a NaN, the
NaN's payload is not compared - the label rule only asks whether a value IS a NaN.)

Every buffer lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.  The vector and the scalar
kernels are both run by the case tables (odd sizes and one-element pointer offsets take the scalar ones) and once more against each
other with IVOSW_IPN_SCALAR=1 in a fresh child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from tests import ipn_ref as ir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 16                                                  # elements in front of and behind every buffer: a multiple of 16 bytes for each type
WEIGHTS = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.7, 0.25, 1.0 - 1.0 / 7.0)          # 1/3, 0.7 and 6/7 do not round-trip through float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _vector_path_unless_asked(monkeypatch):
    monkeypatch.delenv("IVOSW_IPN_SCALAR", raising=False)


class Buf:
    """A device buffer holding `data` (flat) PAD + off elements inside an allocation filled with `fill`; `ptr(first)` addresses element
    `first` of the data; `back()` returns the data as it is now after checking the guard bands."""

    def __init__(self, dev, data, fill, off=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.fill, self.lo, self.n = fill, PAD + off, data.size
        self.host = np.full(data.size + 3 * PAD, fill, data.dtype)
        self.host[self.lo:self.lo + self.n] = data
        self.t = torch.from_numpy(self.host).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, first=0):
        return ctypes.c_void_p(self.t.data_ptr() + (self.lo + first) * self.t.element_size())

    def back(self, name, unchanged=False):
        h = self.t.cpu().numpy()
        bits = lambda a: a.view(np.uint8)
        assert (bits(h[:self.lo]) == bits(self.host[:self.lo])).all() and (bits(h[self.lo + self.n:]) == bits(self.host[self.lo + self.n:])).all(), \
            f"{name}: written outside its extent"
        if unchanged:
            np.testing.assert_array_equal(bits(h), bits(self.host), err_msg=f"{name}: written by a refused call / an input")
        return h[self.lo:self.lo + self.n]


def _same_bits(got, want, why):
    """Equal bit for bit, except that two NaNs are equal whatever their payloads."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, why
    if got.dtype == np.float32:
        both_nan = np.isnan(got) & np.isnan(want)
        got, want = np.where(both_nan, np.float32(0), got).view(np.uint32), np.where(both_nan, np.float32(0), want).view(np.uint32)
    np.testing.assert_array_equal(got, want, err_msg=why)


# ================================================================================================ dilate
DILATE_SIZES = [(1, 1), (2, 7), (5, 5), (9, 33), (17, 64), (33, 70)]
OUT_FILL = 77


def _scribbles(n, H, W, num_objects):
    """n sparse maps: -1 everywhere but a scribble pixel in every corner and in the middle of every edge, two objects within two pixels
    of each other, values outside -1 .. num_objects (they count as -1) and a sparse random rest."""
    rng = np.random.default_rng(1000 * H + 10 * W + num_objects)
    m = np.where(rng.random((n, H, W)) < 0.04, rng.integers(0, num_objects + 1, (n, H, W)), -1).astype(np.int8)
    top = num_objects
    for k in range(n):
        m[k, 0, 0], m[k, 0, W - 1], m[k, H - 1, 0], m[k, H - 1, W - 1] = top, 0, 0, top                      # corners
        m[k, 0, W // 2], m[k, H - 1, W // 2], m[k, H // 2, 0], m[k, H // 2, W - 1] = top, 0, top, 0          # edges
        if H >= 5 and W >= 5:
            y, x = H // 2, max(W // 2 - 1, 2)
            m[k, y - 1:y + 2, x - 2:x + 3] = -1
            m[k, y, x], m[k, y, x + 2] = top, max(top - 1, 0)                                               # two pixels apart
            m[k, y + 1, x + 1] = (num_objects + 1, 127, -2, -128)[k % 4]                                     # out of range, between them
        if H >= 9:
            m[k, 1, 2:6] = (num_objects + 1, 127, -2, -128)
    if H == 1 and W == 1:
        m[1:] = -1                                        # a map with nothing in it
    return m


def _dilate(dev, m, num_objects, off=(0, 0), **geom):
    n, H, W = m.shape
    src, dst = Buf(dev, m, 0, off[0]), Buf(dev, np.full(m.size, OUT_FILL, np.int8), OUT_FILL, off[1])    # input guard: object 0, a value that WOULD spread
    g = dict(n=n, H=H, W=W, num_objects=num_objects, mask=src.ptr(), out=dst.ptr())
    g.update(geom)
    rc = L.lib().ivosw_ipn_dilate(g["mask"], g["n"], g["H"], g["W"], g["num_objects"], g["out"], L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    src.back("mask", unchanged=True)
    return rc, dst.back("out", unchanged=rc != 0).reshape(m.shape), (src, dst)


@pytest.mark.parametrize("H,W", DILATE_SIZES, ids=lambda v: str(v))
def test_dilate_case_table(dev, monkeypatch, H, W):
    for n in (1, 3):
        for num_objects in (0, 1, 3):
            m = _scribbles(n, H, W, num_objects)
            want = ir.dilate_diamond(m, num_objects)
            for k in range(n):                            # the reference's literal loop, map by map
                np.testing.assert_array_equal(ir.dilate_ref(m[k], num_objects), want[k])
            rc, got, _ = _dilate(dev, m, num_objects)
            assert rc == 0, L.lib().ivosw_last_error()
            assert got.dtype == np.int8
            np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f"n={n} num_objects={num_objects}")
            assert (want[0] >= 0).any() and ((m > num_objects) | (m < -1)).any() == (H >= 5 and W >= 5)
            if n == 3 and num_objects == 3:
                for off in ((1, 0), (0, 1), (2, 2), (3, 1), (4, 4)):          # an unaligned base pointer: the scalar kernel
                    rc, o, _ = _dilate(dev, m, num_objects, off=off)
                    assert rc == 0
                    np.testing.assert_array_equal(o, got, err_msg=f"offset {off}")
                monkeypatch.setenv("IVOSW_IPN_SCALAR", "1")                   # read by the launcher at every call
                rc, o, _ = _dilate(dev, m, num_objects)
                monkeypatch.delenv("IVOSW_IPN_SCALAR")
                assert rc == 0
                np.testing.assert_array_equal(o, got, err_msg="IVOSW_IPN_SCALAR")


def test_dilate_two_objects_within_two_pixels(dev):
    """The larger object wins wherever both reach; where only the smaller reaches, it stays."""
    m = np.full((1, 9, 16), -1, np.int8)
    m[0, 4, 5], m[0, 4, 7] = 1, 2
    rc, got, _ = _dilate(dev, m, 2)
    assert rc == 0
    assert got[0, 4, 6] == 2 and got[0, 4, 5] == 2 and got[0, 4, 4] == 1 and got[0, 4, 3] == 1 and got[0, 4, 9] == 2 and got[0, 4, 2] == -1
    assert got[0, 2, 5] == 1 and got[0, 2, 7] == 2 and got[0, 3, 6] == 2 and got[0, 1, 5] == -1
    np.testing.assert_array_equal(got.astype(np.int64), ir.dilate_diamond(m, 2))
    rc, got1, _ = _dilate(dev, m, 1)                      # object 2 is out of range now: it counts as -1, it does not block object 1
    assert rc == 0 and got1[0, 4, 6] == 1 and got1[0, 4, 7] == 1 and got1[0, 4, 8] == -1
    np.testing.assert_array_equal(got1.astype(np.int64), ir.dilate_diamond(m, 1))


def test_dilate_refusals_write_nothing(dev):
    m = _scribbles(2, 9, 32, 3)
    err = lambda: L.lib().ivosw_last_error()
    for geom, text in ((dict(n=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-3), b"bad shape"), (dict(num_objects=-1), b"[0, 126]"),
                       (dict(num_objects=127), b"[0, 126]"), (dict(H=1 << 16, W=1 << 15), b"too large"), (dict(mask=None), b"null mask"),
                       (dict(out=None), b"null out")):
        rc, _, _ = _dilate(dev, m, geom.pop("num_objects", 3), **geom)        # (_dilate asserts that both buffers are what they were)
        assert rc == -1 and text in err(), (geom, err())
    src = Buf(dev, m, 0)
    rc = L.lib().ivosw_ipn_dilate(src.ptr(), 2, 9, 32, 3, src.ptr(), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    src.back("mask", unchanged=True)
    assert rc == -1 and b"must not be mask" in err()


# ================================================================================================ merge
FILL = {"E": -3.0, "prev": -5.0, "probs": -7.0, "u8": 77, "f32": -7.0}
OUTS = ("probs", "u8", "f32")
SMALL = [(K, T, H, W) for K in (1, 2, 4, 11) for T in (1, 3) for H, W in ((4, 4), (5, 7), (16, 20))]
LONG = [(K, T, 4, 4) for K in (1, 2, 4, 11) for T in (257, 300)]          # across the 256-frames-per-launch boundary
_DATA = {}


def _index(K):
    return [(j + 1) % K for j in range(K)] if K < 4 else [2, 0, 3, 1] + list(range(K - 1, 3, -1))


def _data(K, T, H, W):
    """(E, prev, weight) of a case, seeded; made once and never written.  Exact ties between channels (before and after the blend), a
    -0.0 against a 0.0 above negative rest, and - for K > 1 - a plane of NaNs and a pixel where two channels are NaN."""
    key = (K, T, H, W)
    if key not in _DATA:
        rng = np.random.default_rng(K * 100003 + T * 1009 + H * 31 + W)
        E = rng.standard_normal((K, T, H, W)).astype(np.float32)
        prev = rng.standard_normal((K, T, H, W)).astype(np.float32)
        if K > 1:
            for a in (E, prev):
                a[1, :, 0, :2] = a[0, :, 0, :2] = np.abs(a[0, :, 0, :2]) + 10          # positions 0 and 1 tie at the top
                a[:, :, 1, 1] = a[0, :, 1, 1][None]                                  # every channel ties
                a[:, :, 2, 0] = -1.0
                a[0, :, 2, 0], a[1, :, 2, 0] = -0.0, 0.0
            E[K - 1, 0] = np.nan                                                     # a NaN plane: that channel wins the whole frame
            E[0, 0, 3, 3] = np.nan                                                   # ... except where an earlier canonical channel is NaN too
        weight = [WEIGHTS[(f + K) % len(WEIGHTS)] for f in range(T)]
        E.setflags(write=False)
        prev.setflags(write=False)
        _DATA[key] = (E, prev, weight)
    return _DATA[key]


def _merge(dev, E, prev, weight, index, want=OUTS, off=None, over=None):
    """ivosw_ipn_merge -> (rc, {name: numpy}).  prev None: prev_E = NULL.  index None: NULL.  Every buffer lies PAD elements inside an
    allocation of its own, moved by off[name] further elements (0: 16-byte aligned)."""
    off = off or {}
    K, T, H, W = E.shape
    n = T * H * W
    bufs = {"E": Buf(dev, E, FILL["E"], off.get("E", 0))}
    if prev is not None:
        bufs["prev"] = Buf(dev, prev, FILL["prev"], off.get("prev", 0))
    shapes = {"E": E.shape, "prev": E.shape, "probs": E.shape, "u8": (T, H, W), "f32": (T, H, W)}
    for name, dt, size in (("probs", np.float32, K * n), ("u8", np.uint8, n), ("f32", np.float32, n)):
        if name in want:
            bufs[name] = Buf(dev, np.full(size, FILL[name], dt), FILL[name], off.get(name, 0))
    wn, wo = ir.weights32(weight) if weight is not None else (None, None)
    fp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    wn, wo = (None if a is None else np.ascontiguousarray(a) for a in (wn, wo))
    ptr = lambda name: bufs[name].ptr() if name in bufs else None
    g = dict(E=ptr("E"), prev=ptr("prev"), K=K, T=T, H=H, W=W, wn=fp(wn), wo=fp(wo), index=None if index is None else L.int_array(index),
             probs=ptr("probs"), sc=n, u8=ptr("u8"), f32=ptr("f32"))
    g.update(over or {})
    rc = L.lib().ivosw_ipn_merge(g["E"], g["prev"], g["K"], g["T"], g["H"], g["W"], g["wn"], g["wo"], g["index"], g["probs"], g["sc"], g["u8"],
                                 g["f32"], L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    out = {}
    for name, b in bufs.items():
        h = b.back(name, unchanged=rc != 0 or name == "prev" or (name == "E" and g["prev"] is None))
        if name != "prev":
            out[name] = h.reshape(shapes[name])
    return rc, out


def _check_merge(out, E, prev, weight, index, why):
    merged = E if prev is None else ir.blend32(E, prev, weight)
    idx = list(range(E.shape[0])) if index is None else index
    _same_bits(out["E"], merged, f"{why}: all_E")
    if "probs" in out:
        _same_bits(out["probs"], ir.canonical(merged, idx), f"{why}: probs")
    lab = ir.labels_ref(merged, idx)
    if "u8" in out:
        np.testing.assert_array_equal(out["u8"], lab, err_msg=f"{why}: label_u8")
    if "f32" in out:
        _same_bits(out["f32"], lab.astype(np.float32), f"{why}: label_f32")
    return lab


def _variants(K):
    for with_prev in (False, True):
        for index in ((None,) if K == 1 else (None, _index(K))):
            yield with_prev, index


@pytest.mark.parametrize("K,T,H,W", SMALL + LONG, ids=lambda v: str(v))
def test_merge_case_table(dev, K, T, H, W):
    """With and without prev_E, identity and permuted channel order, probs NULL and not, label-only - against the references."""
    E, prev, weight = _data(K, T, H, W)
    for with_prev, index in _variants(K):
        p, w = (prev, weight) if with_prev else (None, None)
        why = f"prev={with_prev} index={index}"
        rc, out = _merge(dev, E, p, w, index)
        assert rc == 0, L.lib().ivosw_last_error()
        lab = _check_merge(out, E, p, w, index, why)
        if K > 1 and not with_prev:
            canon_of_last = (list(range(K)) if index is None else index)[K - 1]
            canon_of_first = (list(range(K)) if index is None else index)[0]
            assert lab[0, 3, 3] == min(canon_of_last, canon_of_first) and (np.delete(lab[0].reshape(-1), 3 * W + 3) == canon_of_last).all()   # NaN: the first one
            assert (lab[1:, 0, :2] == min(index[0], index[1]) if index else lab[1:, 0, :2] == 0).all()       # ties: the first maximum
        # probs = NULL (what the host passes for the identity) and the label-only forms give the same bits in what they do write
        for sub in (("u8", "f32"), ("u8",), ("f32",), ("probs",)) + (((),) if with_prev else ()):
            rc, got = _merge(dev, E, p, w, index, want=sub)
            assert rc == 0, (sub, L.lib().ivosw_last_error())
            assert set(got) == set(sub) | {"E"}
            for name in got:
                _same_bits(got[name], out[name], f"{why}: {name} alone in {sub}")


@pytest.mark.parametrize("K,T,H,W", [(4, 3, 16, 20), (2, 3, 4, 4), (11, 257, 4, 4)], ids=lambda v: str(v))
def test_merge_offset_pointers_and_the_scalar_switch(dev, monkeypatch, K, T, H, W):
    """A one-element offset of any pointer, or a channel stride off the 16-byte grid, takes the scalar kernel: the same bits."""
    E, prev, weight = _data(K, T, H, W)
    index = _index(K)
    rc, base = _merge(dev, E, prev, weight, index)
    assert rc == 0
    for off in ({"E": 1}, {"prev": 1}, {"probs": 1}, {"u8": 1}, {"u8": 2}, {"f32": 1}, {"E": 3, "prev": 2, "probs": 3, "u8": 3, "f32": 2},
                {"E": 4, "prev": 4, "probs": 4, "u8": 4, "f32": 4}):
        rc, got = _merge(dev, E, prev, weight, index, off=off)
        assert rc == 0
        for name in base:
            _same_bits(got[name], base[name], f"offset {off}: {name}")
    monkeypatch.setenv("IVOSW_IPN_SCALAR", "1")           # read by the launcher at every call
    rc, got = _merge(dev, E, prev, weight, index)
    monkeypatch.delenv("IVOSW_IPN_SCALAR")
    assert rc == 0
    for name in base:
        _same_bits(got[name], base[name], f"IVOSW_IPN_SCALAR: {name}")
    # a wider channel stride, on and off the 16-byte grid: the planes land at the stride, the gaps keep their fill
    n = T * H * W
    for sc in (n + 4, n + 1):
        wide = Buf(dev, np.full((K - 1) * sc + n, FILL["probs"], np.float32), FILL["probs"])
        rc, got = _merge(dev, E, prev, weight, index, want=("u8",), over=dict(probs=wide.ptr(), sc=sc))
        assert rc == 0
        h = wide.back("wide probs")
        for i in range(K):
            _same_bits(h[i * sc:i * sc + n].reshape(T, H, W), base["probs"][i], f"stride {sc}: channel {i}")
            assert i == K - 1 or (h[i * sc + n:(i + 1) * sc] == FILL["probs"]).all()


CHILD_CASES = [(4, 3, 16, 20), (11, 300, 4, 4)]


def child_main(path):
    """Runs in the child process of the test below (IVOSW_IPN_SCALAR=1 in its environment from the start)."""
    assert os.environ.get("IVOSW_IPN_SCALAR") == "1"
    dev = torch.device("cuda:0")
    out = {}
    for c, (K, T, H, W) in enumerate(CHILD_CASES):
        E, prev, weight = _data(K, T, H, W)
        rc, got = _merge(dev, E, prev, weight, _index(K))
        assert rc == 0
        out.update({f"merge{c}_{k}": v for k, v in got.items()})
        m = _scribbles(3, 17, 64, 3)
        rc, d, _ = _dilate(dev, m, 3)
        assert rc == 0
        out[f"dilate{c}"] = d
    np.savez(path, **out)


def test_scalar_kernels_in_a_fresh_process(dev, tmp_path):
    path = str(tmp_path / "scalar.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, IVOSW_IPN_SCALAR="1")
    r = subprocess.run([sys.executable, "-c", f"from tests import test_gpu_ipn_glue as t; t.child_main({path!r})"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sca = np.load(path)
    for c, (K, T, H, W) in enumerate(CHILD_CASES):
        E, prev, weight = _data(K, T, H, W)
        rc, vec = _merge(dev, E, prev, weight, _index(K))
        assert rc == 0
        _check_merge(vec, E, prev, weight, _index(K), "vector")
        for name in vec:
            _same_bits(sca[f"merge{c}_{name}"], vec[name], f"child {c}: {name}")
        rc, d, _ = _dilate(dev, _scribbles(3, 17, 64, 3), 3)
        assert rc == 0
        np.testing.assert_array_equal(sca[f"dilate{c}"], d)


def test_merge_refusals_write_nothing(dev):
    K, T, H, W = 4, 3, 4, 4
    E, prev, weight = _data(K, T, H, W)
    n = T * H * W
    err = lambda: L.lib().ivosw_last_error()
    bad = lambda *v: L.int_array(v)
    for over, text in ((dict(K=0), b"[1, 32]"), (dict(K=33), b"[1, 32]"), (dict(T=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=0), b"bad shape"),
                       (dict(H=1 << 16, W=1 << 15), b"too large"), (dict(T=1 << 30, H=1 << 10, W=1 << 10), b"2^40"),
                       (dict(index=bad(0, 1, 2, 2)), b"not a permutation"), (dict(index=bad(0, 1, 2, 4)), b"not a permutation"),
                       (dict(index=bad(-1, 0, 1, 2)), b"not a permutation"), (dict(wn=None), b"needs w_new32"), (dict(wo=None), b"needs w_new32"),
                       (dict(sc=n - 1), b"channels overlap"), (dict(E=None), b"null all_E")):
        rc, _ = _merge(dev, E, prev, weight, None, over=over)          # (_merge asserts that every buffer is what it was)
        assert rc == -1 and text in err(), (over, err())
    rc, _ = _merge(dev, E, None, None, None, want=())
    assert rc == -1 and b"no output" in err()
    # probs inside all_E, and ending one element into it
    e = Buf(dev, np.tile(E.reshape(-1), 2), FILL["E"])                  # 2 * K * n elements: the second half stands for all_E
    for first, sc in ((K * n, n), (0, n + 1), (K * n - 1, n)):
        rc = L.lib().ivosw_ipn_merge(e.ptr(K * n), None, K, T, H, W, None, None, None, e.ptr(first), sc, None, None, L.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        e.back("all_E", unchanged=True)
        assert rc == -1 and b"overlaps all_E" in err(), (first, sc, err())
    rc = L.lib().ivosw_ipn_merge(e.ptr(K * n), None, K, T, H, W, None, None, bad(1, 0, 3, 2), e.ptr(0), n, None, None, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0, err()                                              # probs ending exactly where all_E begins is fine
    h = e.back("all_E")
    _same_bits(h[K * n:].reshape(E.shape), E, "all_E")
    _same_bits(h[:K * n].reshape(E.shape), ir.canonical(E, [1, 0, 3, 2]), "probs in front of all_E")
