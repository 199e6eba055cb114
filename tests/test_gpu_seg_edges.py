"""GPU: the segmentation epilogue (csrc/seg_epilogue.hip) through the C ABI against the float64 reference of oracle/seg_ref.py
(pinned on the CPU by tests/test_oracle_seg_ref.py), on a case table that runs every one of the launcher's ten instantiations.

Labels: the float64 argmax wherever the float64 top-two gap exceeds twice the derived bound 7 * 2^-24 * max|tap|; either of the two
best at the remaining pixels, which are at most 1e-3 of a case.

Probabilities: the kernel's largest absolute error against float64 is compared with the error of torch's float32 CPU kernels
(softmax(interpolate(x))) against the same float64 values on the same input:

    err_kernel <= PROB_MULT * err_torch + PROB_FLOOR

PROB_MULT = 3 was chosen after the first run on an MI355X (LAB_NOTES.md, "Segmentation epilogue against float64", has both errors
and the ratio for every case): the largest measured ratio is below 2 - the register kernels' hardware exp2 and single reciprocal
included.  PROB_FLOOR = 2^-24 is half an ulp of a probability in [0.5, 1): below it a ratio of two errors is a ratio of single
roundings.  On the plain inputs the older bar - 2e-6 absolute against torch - is asserted as well.  It is NOT asserted on the offset
(+ 100) and wide (x 20) variants: there torch's own float32 error against float64 is 1e-6 .. 3.4e-6, and two correct float32
evaluations lie up to 5e-6 apart (tests/test_oracle_seg_ref.py shows this on the CPU); on those the comparison above is the bar.
Terms whose float64 value is below float32's smallest normal number are held to an absolute bound only (<= 2^-125).
"""
import ctypes

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import utils_manet
from oracle import seg_ref as sr

pytestmark = pytest.mark.gpu

PROB_MULT = 3.0
PROB_FLOOR = 2.0 ** -24
ALL = ("probs", "i64", "u8", "f32")
PAD = 16                    # elements in front of and behind every output: a multiple of 16 bytes for each type
FILL = {"probs": -7.0, "i64": -7, "u8": 77, "f32": -7.0}
DTYPE = {"probs": torch.float32, "i64": torch.int64, "u8": torch.uint8, "f32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _vector_path_unless_asked(monkeypatch):
    monkeypatch.delenv("IVOSW_SEG_SCALAR", raising=False)


def _run(dev, x, H, W, want=ALL, off=None, strides=None):
    """ivosw_seg_epilogue on logits x (numpy float32 [k,C,hs,ws]) -> (rc, {name: numpy}).  Every requested output lies PAD elements
    inside a buffer of its own, moved by off[name] further elements (0: 16-byte aligned); the elements around it must keep their fill."""
    off = off or {}
    k, C, hs, ws = x.shape
    d_x = torch.from_numpy(x).to(dev)
    sn, sc = strides or (C * H * W, H * W)
    size = {"probs": max(k * C * H * W, (k - 1) * sn + (C - 1) * sc + H * W), "i64": k * H * W, "u8": k * H * W, "f32": k * H * W}      # the extent the strides span
    bufs, ptrs, lo = {}, {}, {}
    for name in ALL:
        ptrs[name] = None
        if name in want:
            buf = torch.full((size[name] + 3 * PAD,), FILL[name], dtype=DTYPE[name], device=dev)
            assert buf.data_ptr() % 16 == 0
            lo[name] = PAD + off.get(name, 0)
            ptrs[name] = ctypes.c_void_p(buf.data_ptr() + lo[name] * buf.element_size())
            bufs[name] = buf
    rc = L.lib().ivosw_seg_epilogue(L.dptr(d_x), k, C, hs, ws, H, W, ptrs["probs"], sn, sc, ptrs["i64"], ptrs["u8"], ptrs["f32"],
                                    L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    out = {}
    for name, buf in bufs.items():
        h = buf.cpu().numpy()
        a, b = lo[name], lo[name] + size[name]
        assert (h[:a] == FILL[name]).all() and (h[b:] == FILL[name]).all(), f"{name}: written outside its extent"
        if rc != 0:
            assert (h == FILL[name]).all(), f"{name}: written by a refused call"
        if name == "probs" and strides and rc == 0:              # the planes where the strides put them; the gaps between them keep their fill
            idx = (np.arange(k)[:, None, None] * sn + np.arange(C)[None, :, None] * sc + np.arange(H * W)[None, None, :]).reshape(-1)
            gaps = np.ones(b - a, bool)
            gaps[idx] = False
            assert (h[a:b][gaps] == FILL[name]).all(), "probs: written between the planes"
            out[name] = h[a:b][idx].reshape(k, C, H, W)
            continue
        out[name] = h[a:a + (k * C * H * W if name == "probs" else size[name])].reshape((k, C, H, W) if name == "probs" else (k, H, W))
    return rc, out


def _assert_same_bits(a, b, why):
    for name in a:
        np.testing.assert_array_equal(a[name].view(np.uint8), b[name].view(np.uint8), err_msg=f"{why}: {name}")


_REF = {}


def _case(c):
    if c.name not in _REF:
        x = sr.case_logits(c)
        _REF[c.name] = (x, sr.reference(x, c.H, c.W), sr.torch_fp32(x, c.H, c.W)[1])
    return _REF[c.name]


def _check_probs(name, got, ref, p_torch, plain):
    err_k = float(np.abs(got.astype(np.float64) - ref.probs).max())
    err_t = float(np.abs(p_torch.astype(np.float64) - ref.probs).max())
    vs_t = float(np.abs(got - p_torch).max())
    print(f"SEGFIG {name} err_kernel={err_k:.3e} err_torch={err_t:.3e} ratio={err_k / err_t if err_t else float('nan'):.2f} vs_torch={vs_t:.3e}")
    assert err_k <= PROB_MULT * err_t + PROB_FLOOR, (err_k, err_t)
    if plain:
        assert vs_t <= 2e-6, vs_t
    tiny = ref.probs < sr.FLT_MIN
    assert (got[tiny] >= 0).all() and (got[tiny] <= 2.0 ** -125).all()
    assert np.isfinite(got).all() and (got >= 0).all() and np.abs(got.astype(np.float64).sum(1) - 1).max() < 1e-5
    return err_k, err_t


@pytest.mark.parametrize("c", sr.CASES, ids=lambda c: c.name)
def test_every_instantiation_against_float64(dev, c):
    x, ref, p_t = _case(c)
    rc, out = _run(dev, x, c.H, c.W)
    assert rc == 0
    sr.check_labels(out["i64"], ref)
    np.testing.assert_array_equal(out["u8"], out["i64"])
    np.testing.assert_array_equal(out["f32"], out["i64"].astype(np.float32))
    _check_probs(c.name, out["probs"], ref, p_t, c.variant == "plain")


def test_one_class(dev):
    """C = 1: every probability exactly 1, every label 0, on the vector and on the scalar path."""
    for H, W in ((8, 10), (7, 9)):
        rc, out = _run(dev, sr.logits(2, 1, 4, 5, seed=1), H, W)
        assert rc == 0 and (out["probs"] == 1.0).all() and (out["i64"] == 0).all() and (out["u8"] == 0).all() and (out["f32"] == 0).all()


@pytest.mark.parametrize("C", [3, 4, 5, 8, 11, 16, 17])
def test_exact_ties_go_to_the_first_maximum(dev, C):
    """Identical planes upsample to identical values: torch.argmax's rule (the first maximum) decides, on every kernel."""
    for H, W in ((12, 13), (9, 9)):
        x = sr.logits(2, C, 5, 6, seed=C)
        x[:, 1:] = x[:, 1:2]
        x[:, 0] = x[:, 1] - 50.0                      # never the best: classes 1 .. C-1 tie exactly, 1 wins
        rc, out = _run(dev, x, H, W)
        assert rc == 0 and (out["i64"] == 1).all() and (out["u8"] == 1).all() and (out["f32"] == 1).all()
        x[:, 0] = x[:, 1]                             # all C tie: 0 wins
        rc, out = _run(dev, x, H, W)
        assert rc == 0 and (out["i64"] == 0).all()
        np.testing.assert_array_equal(out["probs"], np.full_like(out["probs"], np.float32(1.0) / np.float32(C)))


def test_256_classes_with_uint8_labels(dev):
    x = sr.logits_256()
    ref = sr.reference(x, 6, 10)
    rc, out = _run(dev, x, 6, 10)
    assert rc == 0
    sr.check_labels(out["u8"], ref)
    assert out["u8"][0, 5, 9] == 255 and {0, 128, 255} <= set(np.unique(out["u8"]).tolist())
    np.testing.assert_array_equal(out["i64"], out["u8"])
    _check_probs("c256", out["probs"], ref, sr.torch_fp32(x, 6, 10)[1], True)
    x257 = np.concatenate([x, x[:, :1] - 5.0], axis=1)
    rc, _ = _run(dev, x257, 6, 10)
    assert rc == -1 and b"C <= 256" in L.lib().ivosw_last_error()
    rc, out = _run(dev, x257, 6, 10, want=("probs", "i64"))         # without uint8 labels 257 classes are fine
    assert rc == 0
    sr.check_labels(out["i64"], sr.reference(x257, 6, 10))


VECTOR_CASES = [c for c in sr.CASES if ",4" in c.kernel]


@pytest.mark.parametrize("c", VECTOR_CASES, ids=lambda c: c.name)
def test_vector_and_scalar_kernels_agree_bit_for_bit(dev, monkeypatch, c):
    x, _, _ = _case(c)
    rc, vec = _run(dev, x, c.H, c.W)
    assert rc == 0
    monkeypatch.setenv("IVOSW_SEG_SCALAR", "1")                    # read by the launcher at every call
    rc, sca = _run(dev, x, c.H, c.W)
    assert rc == 0
    _assert_same_bits(vec, sca, "IVOSW_SEG_SCALAR")


@pytest.mark.parametrize("name", ["full4", "c5_v4", "full16", "column_target"])
def test_misaligned_outputs_take_the_scalar_kernel(dev, name):
    c = [c for c in sr.CASES if c.name == name][0]
    x, _, _ = _case(c)
    rc, want = _run(dev, x, c.H, c.W)
    assert rc == 0
    for off in ({"u8": 1}, {"u8": 2}, {"probs": 1}, {"f32": 1}, {"i64": 1}, {"u8": 3, "probs": 3, "f32": 2}):
        rc, got = _run(dev, x, c.H, c.W, off=off)
        assert rc == 0
        _assert_same_bits(want, got, f"offset {off}")


@pytest.mark.parametrize("name", ["full4", "c11_v4", "c6_v1", "c17"])
def test_outputs_one_at_a_time(dev, name):
    c = [c for c in sr.CASES if c.name == name][0]
    x, _, _ = _case(c)
    rc, want = _run(dev, x, c.H, c.W)
    assert rc == 0
    for one in ALL:
        rc, got = _run(dev, x, c.H, c.W, want=(one,))
        assert rc == 0
        _assert_same_bits({one: want[one]}, got, "alone")
    rc, _ = _run(dev, x, c.H, c.W, want=())
    assert rc == -1 and b"no output" in L.lib().ivosw_last_error()


def test_prob_store_slot_on_the_vector_path(dev):
    """k = 3 frames into frames 2..4 of a 7-frame ProbStore, C = 4, 12 x 13 (h * w % 4 == 0: V = 4 with object-major strides)."""
    k, C, h, w, n_total, frame = 3, 4, 12, 13, 7, 2
    x = sr.logits(k, C, 9, 11, seed=77)
    ref = sr.reference(x, h, w)
    store = utils_manet.ProbStore(n_total, C, h, w, dev)
    store.buf.fill_(-7.0)
    store.labels_u8.fill_(77)
    store.final_masks.fill_(-7.0)
    assert store.buf.data_ptr() % 16 == 0 and (h * w) % 4 == 0
    lab, slot = utils_manet.seg_epilogue(torch.from_numpy(x).to(dev), h, w, store, frame)
    torch.cuda.synchronize(dev)
    inside = slice(frame, frame + k)
    outside = [n for n in range(n_total) if not frame <= n < frame + k]
    assert (store.buf[:, outside] == -7.0).all() and (store.labels_u8[outside] == 77).all() and (store.final_masks[outside] == -7.0).all()
    sr.check_labels(lab.cpu().numpy(), ref)
    np.testing.assert_array_equal(store.labels_u8[inside].cpu().numpy(), lab.cpu().numpy())
    np.testing.assert_array_equal(store.final_masks[inside].cpu().numpy(), lab.float().cpu().numpy())
    got = store.all_P[inside].cpu().numpy()
    np.testing.assert_array_equal(slot.cpu().numpy(), got)
    _check_probs("prob_store", got, ref, sr.torch_fp32(x, h, w)[1], True)
    # the same values as the dense layout gives, bit for bit
    rc, dense = _run(dev, x, h, w, want=("probs",))
    assert rc == 0
    np.testing.assert_array_equal(got.view(np.uint8), dense["probs"].view(np.uint8))


@pytest.mark.parametrize("C", [3, 4])
def test_probability_strides_off_the_grid_take_the_scalar_kernel(dev, C):
    """4 x 8 (H * W % 4 == 0), every pointer 16-byte aligned: a channel or a frame stride that is no multiple of 4 floats puts planes on
    4-byte-aligned bases, so the call runs one pixel per lane - the bits of the dense call (4 pixels per lane), the gaps between the
    planes and the guard bands untouched.  A padded stride that IS a multiple of 4 stays on the vector kernel: the same bits again."""
    k, H, W = 2, 4, 8
    hw = H * W
    x = sr.logits(k, C, 3, 5, seed=40 + C)
    rc, dense = _run(dev, x, H, W)
    assert rc == 0
    for strides in ((C * (hw + 1), hw + 1), (C * hw + 2, hw), (C * hw + 3, hw), (C * (hw + 4), hw + 4)):
        rc, got = _run(dev, x, H, W, strides=strides)
        assert rc == 0, L.lib().ivosw_last_error()
        _assert_same_bits(dense, got, f"strides {strides}")


def test_overlapping_strides_are_refused(dev):
    x = sr.logits(2, 4, 9, 11, seed=5)
    H, W = 12, 13
    for strides in ((4 * H * W, H * W - 4), (H * W - 4, 2 * H * W), (4 * H * W, H * W - 1)):
        rc, _ = _run(dev, x, H, W, strides=strides)
        assert rc == -1 and b"strides overlap" in L.lib().ivosw_last_error()
