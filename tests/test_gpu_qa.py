"""GPU: the assessment-sample path through the C ABI - ivosw_qa_quantize, ivosw_qa_counts_videos, ivosw_qa_targets - with a guard band
behind every output, and the host chain on top (metrics.quantize_probs / qa_targets, misc.save_seg_preds, utils_agent.assess_report, the
save_probs / qa_report keys).  Every comparison is exact: bytes, integers or float bits (tests/qa_ref.py restates the rules)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import metrics
from ivos_w_amd.utils import misc, utils_agent, utils_manet
from oracle import jf_oracle
from tests import qa_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    return L.lib()


# ---------------------------------------------------------------------------------------------- quantise
# (H, W): 5 x 7 scalar (35 % 4 != 0), 4 x 8 vector, 33 x 65 scalar with nine blocks, 32 x 72 vector with three blocks (the last partial)
QUANT_SHAPES = [(5, 7), (4, 8), (33, 65), (32, 72)]
QUANT_CASES = [(H, W, O, n, layout, off) for (H, W) in QUANT_SHAPES for (O, n) in ((1, 1), (3, 3), (1, 3), (3, 1))
               for layout in ("reference", "store") for off in (0, 1)]


def _quant_input(H, W, O, n, layout, k):
    """float32 [n, O+1, H, W] on the deciding value grid, channel 0 NaN; returned in the memory order of `layout`."""
    a = R.fill((n, O + 1, H, W), np.random.default_rng(k))
    a[:, 0] = np.nan
    mem = a if layout == "reference" else np.ascontiguousarray(a.transpose(1, 0, 2, 3))
    return a, mem


def _quantize_abi(lib, dev, H, W, O, n, layout, off, k):
    """One ivosw_qa_quantize call; `off` floats in front of the base (off = 1: a base 4 bytes off the 16-byte grid).  -> (bytes, want)."""
    a, mem = _quant_input(H, W, O, n, layout, k)
    flat = torch.full((mem.size + 4,), float("nan"), dtype=torch.float32, device=dev)
    flat[off:off + mem.size] = torch.from_numpy(mem.reshape(-1)).to(dev)
    hw = H * W
    sn, sc = ((O + 1) * hw, hw) if layout == "reference" else (hw, n * hw)
    out = torch.full((O * n * hw + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    L.check(lib.ivosw_qa_quantize(ctypes.c_void_p(flat.data_ptr() + 4 * off), n, O, H, W, sn, sc, L.dptr(out), L.stream_ptr(dev)), "qa_quantize")
    got = out.cpu().numpy()
    assert (got[O * n * hw:] == 0xA5).all(), "the guard band behind the planes was written"
    return got[:O * n * hw].reshape(O, n, H, W), R.quantize_probs(a, O)


def scalar_child(path):
    """Run in a child process with IVOSW_QA_SCALAR set: every quantise case through the scalar instantiation, saved to `path`."""
    assert os.environ.get("IVOSW_QA_SCALAR")
    dev, lib = torch.device("cuda", 0), L.lib()
    np.savez(path, **{f"c{k}": _quantize_abi(lib, dev, *case, k)[0] for k, case in enumerate(QUANT_CASES)})


@pytest.fixture(scope="module")
def scalar_results(dev, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("qa") / "scalar.npz")
    env = dict(os.environ, IVOSW_QA_SCALAR="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", f"import ivos_w_amd; from tests.test_gpu_qa import scalar_child; scalar_child({path!r})"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(path)


@pytest.mark.parametrize("k", range(len(QUANT_CASES)), ids=lambda k: "{}x{}-O{}-n{}-{}-off{}".format(*QUANT_CASES[k]))
def test_quantize_vector_scalar_and_restatement_agree(lib, dev, scalar_results, k):
    got, want = _quantize_abi(lib, dev, *QUANT_CASES[k], k)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(scalar_results[f"c{k}"], want)


@pytest.mark.parametrize("pad_c,pad_n,plane_off", [(1, 0, 0), (0, 2, 0), (0, 0, 1)], ids=["stride_c", "stride_n", "planes_off"])
def test_quantize_stride_or_planes_off_the_grid_take_the_scalar_kernel(lib, dev, pad_c, pad_n, plane_off):
    """4 x 8 (H * W % 4 == 0) on a 16-byte aligned base: a channel or frame stride that is no multiple of 4 floats, or planes one byte
    off the 4-byte grid, run one pixel per lane - the bytes of the aligned dense call, nothing behind the planes."""
    H, W, O, n = 4, 8, 2, 3
    hw = H * W
    a, _ = _quant_input(H, W, O, n, "reference", 99)
    sc = hw + pad_c
    sn = (O + 1) * sc + pad_n
    mem = np.full(n * sn, np.nan, np.float32)
    for f in range(n):
        for c in range(O + 1):
            mem[f * sn + c * sc:f * sn + c * sc + hw] = a[f, c].reshape(-1)
    src = torch.from_numpy(mem).to(dev)
    out = torch.full((4 + O * n * hw + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    L.check(lib.ivosw_qa_quantize(L.dptr(src), n, O, H, W, sn, sc, ctypes.c_void_p(out.data_ptr() + plane_off), L.stream_ptr(dev)), "qa_quantize")
    got = out.cpu().numpy()
    assert (got[:plane_off] == 0xA5).all() and (got[plane_off + O * n * hw:] == 0xA5).all(), "written outside the planes"
    dense, want = _quantize_abi(lib, dev, H, W, O, n, "reference", 0, 99)
    np.testing.assert_array_equal(got[plane_off:plane_off + O * n * hw].reshape(O, n, H, W), want)
    np.testing.assert_array_equal(dense, want)


def test_quantize_covers_every_byte_and_the_specials(lib, dev):
    g = R.value_grid()
    pad = (-g.size) % 4
    a = np.concatenate([g, np.zeros(pad, np.float32)]).reshape(1, 1, 1, -1)
    p = torch.from_numpy(np.concatenate([np.full_like(a, np.nan), a], 1)).to(dev)
    q = metrics.quantize_probs(p, 1).cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(q, R.quantize(a.reshape(-1)))
    assert set(q.tolist()) == set(range(256))


def test_quantize_refusals(lib, dev):
    p = torch.zeros(2 * 3 * 16, dtype=torch.float32, device=dev)
    out = torch.full((64 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    st = L.stream_ptr(dev)
    ok = (L.dptr(p), 2, 2, 4, 4, 48, 16, L.dptr(out), st)
    for i, bad in ((0, None), (7, None), (1, 0), (2, 0), (3, 0), (4, 0), (5, 15), (6, 15), (1, 65536), (2, 65536)):
        args = list(ok)
        args[i] = bad
        assert lib.ivosw_qa_quantize(*args) == -1, (i, bad)
        assert b"ivosw_qa_quantize" in lib.ivosw_last_error()
    torch.cuda.synchronize(dev)
    assert bool((out == 0xA5).all())
    L.check(lib.ivosw_qa_quantize(*ok), "qa_quantize")
    assert bool((out[:64] == 0).all()) and bool((out[64:] == 0xA5).all())


def test_quantize_probs_accepts_both_layouts_stores_and_host_arrays(dev):
    a, _ = _quant_input(6, 10, 2, 3, "reference", 5)
    want = R.quantize_probs(a, 2)
    ref = torch.from_numpy(a).to(dev)
    store = utils_manet.ProbStore(3, 3, 6, 10, dev)
    store.buf.copy_(ref.permute(1, 0, 2, 3))
    for src in (ref, store.all_P, store, a):
        np.testing.assert_array_equal(metrics.quantize_probs(src, 2).cpu().numpy(), want)
    np.testing.assert_array_equal(metrics.quantize_probs(ref, 1).cpu().numpy(), want[:1])
    with pytest.raises(ValueError, match="objects do not fit"):
        metrics.quantize_probs(ref, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.quantize_probs(torch.from_numpy(a), 2)


# ---------------------------------------------------------------------------------------------- counts from planes
def _bound_pix(H, W):
    return int(metrics.bound_pixels((H, W)))


def _blocky(rng, values, n, H, W):
    cell = max(1, min(H, max(W // 8, 1), 6))
    coarse = rng.integers(0, len(values), (n, -(-H // cell), -(-W // cell)))
    return np.asarray(values, dtype=np.uint8)[np.kron(coarse, np.ones((1, cell, cell), dtype=np.int64))[:, :H, :W]]


SEAM_COLS = (0, 1, 14, 15, 16, 17, 31, 32, 1006, 1007, 1008, 1009, 1022, 1023, 1024, 1025)
SEAM_VALUES = (204, 205, 0, 255)


def _seam(plane, shift):
    """Bytes on both sides of the threshold at the first and last column, around the lane-62 | 63 (1007 | 1008) and segment (1023 | 1024)
    seams, and along the last row - the value pattern moves with `shift`, so objects and frames differ."""
    n, H, W = plane.shape
    cols = sorted({c for c in SEAM_COLS + (W - 2, W - 1) if 0 <= c < W})
    for f in range(n):
        for y in range(H):
            for j, c in enumerate(cols):
                plane[f, y, c] = SEAM_VALUES[(j + y + f + shift) % 4]
        for x in range(W):
            plane[f, H - 1, x] = SEAM_VALUES[(x // 3 + f + shift) % 4]
    return plane


def _plane_video(rng, n, H, W, ids, overlap=True):
    """gt uint8 [n,H,W] and planes uint8 [O,n,H,W]: blocky bytes around the threshold with the seams set; with `overlap` object 2's plane
    repeats object 1's above-threshold pixels over half the picture, so the same pixel is foreground in two planes."""
    gt = _blocky(rng, [0] + list(ids), n, H, W)
    planes = np.stack([_seam(_blocky(rng, [0, 100, 204, 205, 230, 255], n, H, W), o) for o in range(len(ids))])
    if overlap and len(ids) > 1:
        half = planes[0][:, :, :max(W // 2, 1)]
        planes[1][:, :, :max(W // 2, 1)] = np.maximum(planes[1][:, :, :max(W // 2, 1)], half)
    return np.ascontiguousarray(gt), np.ascontiguousarray(planes)


class _Vid:
    def __init__(self, dev, gt, planes, ids, thr=R.THR, bp=None, lead=0):
        """`lead` bytes in front of the planes move the stack off the 16-byte grid (odd W moves every later plane anyway)."""
        self.n, self.H, self.W = gt.shape
        self.ids, self.thr, self.bp = list(ids), thr, _bound_pix(self.H, self.W) if bp is None else bp
        self.gt_np, self.planes_np = gt, planes
        self.gt = torch.from_numpy(gt).to(dev)
        self.buf = torch.zeros(planes.size + lead, dtype=torch.uint8, device=dev)
        self.buf[lead:] = torch.from_numpy(planes.reshape(-1)).to(dev)
        self.planes_ptr = self.buf.data_ptr() + lead

    def desc(self, planes=True):
        d = L.QaVideo(gt=self.gt.data_ptr(), planes=self.planes_ptr if planes else None, n_frames=self.n, H=self.H, W=self.W,
                      n_obj=len(self.ids), bound_pix=self.bp, thr=self.thr)
        for i, v in enumerate(self.ids):
            d.obj_ids[i] = v
        return d


def _qa_counts(lib, dev, vids):
    table = (L.QaVideo * len(vids))(*[v.desc() for v in vids])
    total = sum(v.n * len(v.ids) * 6 for v in vids)
    nbytes = lib.ivosw_qa_counts_ws_bytes(table, len(vids))
    assert nbytes == sum(lib.ivosw_jf_ws_bytes(v.n, v.H, v.W, len(v.ids)) for v in vids) > 0
    counts = torch.full((total + 6,), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.ivosw_qa_counts_videos(table, len(vids), L.dptr(counts), L.dptr(ws), nbytes, L.stream_ptr(dev)), "qa_counts_videos")
    got = counts.cpu().numpy()
    assert (got[total:] == SENTINEL).all(), "the guard band behind the counts was written"
    out, off = [], 0
    for v in vids:
        size = v.n * len(v.ids) * 6
        out.append(got[off:off + size].reshape(v.n, len(v.ids), 6))
        off += size
    return out


def _assert_oracle(v, counts):
    """The J and F the host expressions form from the counts equal the oracle's on per-object binary maps (nb_objects = 1); the two
    area counts are checked as integers too."""
    for o, oid in enumerate(v.ids):
        g = (v.gt_np == oid).astype(np.uint8)
        p = (v.planes_np[o] >= v.thr).astype(np.uint8)
        np.testing.assert_array_equal(counts[:, o, 0], (g & p).reshape(v.n, -1).sum(1))
        np.testing.assert_array_equal(counts[:, o, 1], (g | p).reshape(v.n, -1).sum(1))
        j = jf_oracle.batched_jaccard(g, p, average_over_objects=False, nb_objects=1)[:, 0]
        f = jf_oracle.batched_f_measure(g, p, average_over_objects=False, nb_objects=1, bound_th=v.bp if v.bp >= 1 else 0.008)[:, 0]
        np.testing.assert_array_equal(metrics._jaccard_from(counts[:, o]), j, err_msg=f"J, object {oid}")
        np.testing.assert_array_equal(metrics._f_from(counts[:, o]), f, err_msg=f"F, object {oid}")


# W at the seams of the boundary kernel (16 pixels per lane, 1024-pixel segments) with H at its row seams (4 rows per wave, 16 per block),
# paired so that no case exceeds 20 k pixels
COUNT_SHAPES = [(1, 17), (15, 5), (16, 4), (17, 17), (33, 5), (1009, 4), (1024, 5), (1025, 17), (1041, 17), (1041, 1), (1, 1)]


@pytest.mark.parametrize("W, H", COUNT_SHAPES, ids=lambda v: str(v))
def test_counts_from_overlapping_planes_against_the_oracle(lib, dev, W, H):
    rng = np.random.default_rng(W * 100 + H)
    gt, planes = _plane_video(rng, 2, H, W, [1, 2], overlap=True)
    v = _Vid(dev, gt, planes, [1, 2], lead=1 if W % 2 == 0 else 0)
    assert v.bp >= 1
    counts = _qa_counts(lib, dev, [v])[0]
    if W > 1:
        assert ((planes[0] >= R.THR) & (planes[1] >= R.THR)).any(), "the planes of the two objects must overlap"
        assert {204, 205} <= set(np.unique(planes[:, :, :, [0, W - 1]]).tolist())
    _assert_oracle(v, counts)


@pytest.mark.parametrize("W, H", COUNT_SHAPES, ids=lambda v: str(v))
def test_counts_from_disjoint_planes_equal_the_label_map_pass(lib, dev, W, H):
    """Planes that do not overlap are a label map: six integers equal ivosw_jf_counts on it."""
    rng = np.random.default_rng(W * 100 + H + 7)
    ids = [1, 3, 2]
    gt = _blocky(rng, [0] + ids, 2, H, W)
    pred = np.roll(_blocky(rng, [0] + ids, 2, H, W), 1, axis=2)
    for f in range(2):                                                    # label changes across every seam column and on the last row
        for j, c in enumerate(sorted({c for c in SEAM_COLS + (W - 1,) if c < W})):
            pred[f, :, c] = ([0] + ids)[(j + f) % 4]
        pred[f, H - 1, ::3] = ids[f]
    hi, lo = np.asarray([205, 255, 230], np.uint8), np.asarray([204, 0, 100], np.uint8)
    pick = rng.integers(0, 3, pred.shape)
    planes = np.stack([np.where(pred == oid, hi[pick], lo[pick]) for oid in ids]).astype(np.uint8)
    v = _Vid(dev, np.ascontiguousarray(gt), np.ascontiguousarray(planes), ids, lead=3)
    got = _qa_counts(lib, dev, [v])[0]
    want = torch.empty(2, 3, 6, dtype=torch.int64, device=dev)
    nbytes = lib.ivosw_jf_ws_bytes(2, H, W, 3)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.ivosw_jf_counts(L.dptr(v.gt), L.dptr(torch.from_numpy(np.ascontiguousarray(pred)).to(dev)), 2, H, W, bytes(ids), 3, v.bp,
                                L.dptr(want), L.dptr(ws), nbytes, L.stream_ptr(dev)), "jf_counts")
    np.testing.assert_array_equal(got, want.cpu().numpy())
    assert got.sum() > 0


def test_counts_threshold_is_a_byte_compare(lib, dev):
    """thr = 0 takes every pixel, thr = 255 only the saturated ones, 128 splits at the top bit (the SWAR compare's two halves)."""
    rng = np.random.default_rng(3)
    planes = rng.integers(0, 256, (1, 1, 5, 37), dtype=np.uint8)
    planes[0, 0, 0, :8] = [0, 127, 128, 129, 254, 255, 1, 200]
    gt = np.ones((1, 5, 37), np.uint8)
    for thr in (0, 1, 127, 128, 129, 200, 205, 254, 255):
        c = _qa_counts(lib, dev, [_Vid(dev, gt, planes, [1], thr=thr)])[0]
        assert c[0, 0, 0] == int((planes >= thr).sum()) and c[0, 0, 1] == 5 * 37, thr


def test_counts_mixed_table_equals_the_per_video_calls(lib, dev):
    rng = np.random.default_rng(11)
    specs = [(1, 1, 1, [2], True), (3, 9, 40, [1, 2, 3], True), (1, 17, 1041, [1, 4], True)]
    vids = []
    for k, (n, H, W, ids, ov) in enumerate(specs):
        gt, planes = _plane_video(rng, n, H, W, ids, ov)
        vids.append(_Vid(dev, gt, planes, ids, thr=(205, 128, 205)[k], bp=(0, 1, None)[k], lead=k))
    alone = [_qa_counts(lib, dev, [v])[0] for v in vids]
    for order in ([0, 1, 2], [2, 1, 0], [1, 0, 2]):
        together = _qa_counts(lib, dev, [vids[i] for i in order])
        for i, got in zip(order, together):
            np.testing.assert_array_equal(got, alone[i], err_msg=f"video {i} in order {order}")
    assert all(a.sum() > 0 for a in alone[1:])


def test_counts_refusals_launch_nothing_and_name_the_video(lib, dev):
    rng = np.random.default_rng(2)
    vids = [_Vid(dev, *_plane_video(rng, 1, 4, 9, [1]), [1]) for _ in range(3)]
    counts = torch.full((3 * 6 + 6,), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    st = L.stream_ptr(dev)

    def call(descs, n=None, counts_ptr=L.dptr(counts), ws_ptr=L.dptr(ws), ws_bytes=1 << 16):
        table = (L.QaVideo * len(descs))(*descs)
        return lib.ivosw_qa_counts_videos(table, len(descs) if n is None else n, counts_ptr, ws_ptr, ws_bytes, st), table

    def edited(k, **kw):
        ds = [v.desc() for v in vids]
        for key, val in kw.items():
            setattr(ds[k], key, val)
        return ds
    cases = [(edited(1, planes=None), b"video 1: NULL planes"), (edited(2, gt=None), b"video 2"), (edited(0, n_frames=0), b"video 0"),
             (edited(1, H=0), b"video 1"), (edited(2, W=-1), b"video 2"), (edited(1, n_obj=0), b"video 1"), (edited(1, n_obj=33), b"video 1"),
             (edited(2, bound_pix=33), b"video 2"), (edited(0, bound_pix=-1), b"video 0"), (edited(2, n_frames=65535), b"video 2")]
    for descs, needle in cases:
        rc, table = call(descs)
        assert rc == -1 and needle in lib.ivosw_last_error(), (needle, lib.ivosw_last_error())
        assert lib.ivosw_qa_counts_ws_bytes(table, len(descs)) == 0
    ok = [v.desc() for v in vids]
    assert call(ok, n=0)[0] == -1 and b"n_videos" in lib.ivosw_last_error()
    assert call(ok * 11, n=33)[0] == -1 and b"n_videos" in lib.ivosw_last_error()
    assert call(ok, counts_ptr=None)[0] == -1 and call(ok, ws_ptr=None)[0] == -1
    assert lib.ivosw_qa_counts_videos(None, 3, L.dptr(counts), L.dptr(ws), 1 << 16, st) == -1
    assert call(ok, ws_bytes=16)[0] != 0 and b"workspace" in lib.ivosw_last_error()
    torch.cuda.synchronize(dev)
    assert bool((counts == SENTINEL).all()), "a refused call wrote counts"
    assert call(ok)[0] == 0
    assert bool((counts[:18] != SENTINEL).all()) and bool((counts[18:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- targets and report
def _random_counts(rng, n, O):
    """int64 [n, O, 6] with units on both sides of every branch of the ratio expressions."""
    c = np.zeros((n, O, 6), np.int64)
    c[..., 1] = rng.integers(1, 400, (n, O))
    c[..., 0] = (c[..., 1] * rng.random((n, O))).astype(np.int64)
    c[..., 2], c[..., 3] = rng.integers(1, 60, (n, O)), rng.integers(1, 60, (n, O))
    c[..., 4], c[..., 5] = (c[..., 2] * rng.random((n, O))).astype(np.int64), (c[..., 3] * rng.random((n, O))).astype(np.int64)
    kind = rng.integers(0, 8, (n, O))
    c[kind == 0] = 0                                                       # empty union (and both boundaries empty)
    c[kind == 1, 2] = 0; c[kind == 1, 4] = 0                              # empty pred boundary
    c[kind == 2, 3] = 0; c[kind == 2, 5] = 0                              # empty gt boundary
    c[kind == 3, 4] = 0; c[kind == 3, 5] = 0                              # precision + recall == 0
    return c


def _targets_abi(lib, dev, counts_list, metric, scores=None):
    lengths, n_obj = [c.shape[0] for c in counts_list], [c.shape[1] for c in counts_list]
    units, V = sum(n * o for n, o in zip(lengths, n_obj)), len(counts_list)
    cdev = torch.from_numpy(np.concatenate([c.reshape(-1) for c in counts_list])).to(dev)
    target = torch.full((units + 4,), -3.0, dtype=torch.float64, device=dev)
    valid = torch.full((units + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    loss, diff = (torch.full((V + 4,), -3.0, dtype=torch.float32, device=dev) for _ in range(2))
    n_valid = torch.full((V + 4,), SENTINEL, dtype=torch.int32, device=dev)
    sdev = torch.from_numpy(scores).to(dev) if scores is not None else None
    L.check(lib.ivosw_qa_targets(L.dptr(cdev), L.int_array(n_obj), L.int_array(lengths), V, metrics.METRIC_CODES[metric],
                                 L.dptr(sdev) if sdev is not None else None, L.dptr(target), L.dptr(valid),
                                 L.dptr(loss) if sdev is not None else None, L.dptr(diff) if sdev is not None else None,
                                 L.dptr(n_valid) if sdev is not None else None, L.stream_ptr(dev)), "qa_targets")
    t, v, lo, di, nv = (x.cpu().numpy() for x in (target, valid, loss, diff, n_valid))
    assert (t[units:] == -3.0).all() and (v[units:] == 0xA5).all() and (lo[V:] == -3.0).all() and (di[V:] == -3.0).all() and (nv[V:] == SENTINEL).all()
    if scores is None:
        assert (lo == -3.0).all() and (di == -3.0).all() and (nv == SENTINEL).all()
    return t[:units], v[:units], lo[:V], di[:V], nv[:V]


@pytest.mark.parametrize("metric", ["J", "F", "J_AND_F"])
def test_targets_unit_order_bits_and_report(lib, dev, metric):
    rng = np.random.default_rng(5)
    some = _random_counts(rng, 2, 3)                                      # n_obj = 3, n_frames = 2: a transposed index cannot pass
    some[0, 0] = [3, 4, 5, 6, 2, 3]; some[1, 0] = 0; some[0, 1] = [0, 9, 0, 4, 0, 0]
    some[1, 1] = [1, 9, 4, 0, 0, 0]; some[0, 2] = [2, 7, 3, 3, 0, 0]; some[1, 2] = [7, 7, 5, 5, 5, 5]
    every = _random_counts(rng, 4, 2)
    every[every[..., 1] == 0] = [1, 2, 1, 1, 1, 0]
    none = np.zeros((3, 2, 6), np.int64)
    big = _random_counts(rng, 100, 3)                                     # 300 units: the sum is sequential
    videos = [some, every, none, big, _random_counts(rng, 1, 1)]
    allc = np.concatenate([c.reshape(-1, 6) for c in videos])
    # the inputs cover both sides of every branch
    assert (allc[:, 1] == 0).any() and (allc[:, 1] > 0).any()
    assert ((allc[:, 2] == 0) & (allc[:, 3] > 0)).any() and ((allc[:, 2] > 0) & (allc[:, 3] == 0)).any()
    assert ((allc[:, 2] == 0) & (allc[:, 3] == 0)).any() and ((allc[:, 2] > 0) & (allc[:, 3] > 0)).any()
    assert ((allc[:, 2] > 0) & (allc[:, 3] > 0) & (allc[:, 4] == 0) & (allc[:, 5] == 0)).any()
    want = [R.unit_targets(c, metric) for c in videos]
    wt, wv = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert not np.array_equal(R.unit_targets(some, metric)[0], R.unit_targets(some, metric)[0].reshape(3, 2).T.reshape(-1))
    scores = rng.random(wt.size).astype(np.float32)
    t, v, lo, di, nv = _targets_abi(lib, dev, videos, metric, scores)
    assert t.tobytes() == wt.tobytes()
    np.testing.assert_array_equal(v, wv)
    off = 0
    for k, (tk, vk) in enumerate(want):
        wl, wd, wn = R.reference_loop(scores[off:off + tk.size], tk, vk)
        assert (np.float32(lo[k]).tobytes(), np.float32(di[k]).tobytes(), int(nv[k])) == (wl.tobytes(), wd.tobytes(), wn), (k, lo[k], wl, di[k], wd)
        off += tk.size
    assert int(nv[1]) == 8 and int(nv[2]) == 0 and lo[2] == 0 and di[2] == 0 and 0 < int(nv[0]) < 6 and int(nv[3]) > 200
    # without scores: the same targets, and loss / diff / n_valid are not touched
    t2, v2, _, _, _ = _targets_abi(lib, dev, videos, metric, None)
    assert t2.tobytes() == wt.tobytes() and np.array_equal(v2, wv)


def test_targets_refusals(lib, dev):
    c = torch.zeros(12 * 6, dtype=torch.int64, device=dev)
    t = torch.full((12,), -3.0, dtype=torch.float64, device=dev)
    v = torch.zeros(12, dtype=torch.uint8, device=dev)
    s, lo, di = (torch.zeros(12, dtype=torch.float32, device=dev) for _ in range(3))
    nv = torch.zeros(2, dtype=torch.int32, device=dev)
    st = L.stream_ptr(dev)
    ok = [L.dptr(c), L.int_array([3, 2]), L.int_array([2, 3]), 2, 2, L.dptr(s), L.dptr(t), L.dptr(v), L.dptr(lo), L.dptr(di), L.dptr(nv), st]
    for i, bad, needle in ((0, None, b"null"), (6, None, b"null"), (7, None, b"null"), (8, None, b"go together"), (5, None, b"go together"),
                           (4, 3, b"unknown metric"), (3, 0, b"n_seqs"), (3, 129, b"n_seqs"), (1, L.int_array([3, 0]), b"video 1"),
                           (1, L.int_array([33, 2]), b"video 0"), (2, L.int_array([2, 0]), b"sequence 1")):
        args = list(ok)
        args[i] = bad
        assert lib.ivosw_qa_targets(*args) == -1 and needle in lib.ivosw_last_error(), (i, lib.ivosw_last_error())
    torch.cuda.synchronize(dev)
    assert bool((t == -3.0).all())
    assert lib.ivosw_qa_targets(*ok) == 0
    assert bool((t == 1.0).all())                                        # all counts zero: J = F = 1, nothing valid
    assert nv.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- the chain
def _session(dev, rng, n=4, H=20, W=35, O=3):
    """A small synthetic session: a ProbStore with soft probabilities on both sides of 0.8, its ground truth, and per-unit scores."""
    gt = _blocky(rng, [0, 1, 2, 3][:O + 1], n, H, W)
    logits = rng.normal(0, 3, (n, O + 1, H, W)).astype(np.float32)
    for o in range(1, O + 1):
        logits[:, o] += 4.0 * (np.roll(gt, o, axis=2) == o)
    e = np.exp(logits - logits.max(1, keepdims=True))
    probs = (e / e.sum(1, keepdims=True)).astype(np.float32)
    probs[:, O, :, :3] = 0.0                                              # object O is empty in the first columns
    store = utils_manet.ProbStore(n, O + 1, H, W, dev)
    store.buf.copy_(torch.from_numpy(probs).to(dev).permute(1, 0, 2, 3))
    scores = torch.from_numpy(rng.random((O, n)).astype(np.float32)).to(dev)
    return gt, probs, store, scores


def _read_gray(path):
    if path.endswith(".png"):
        from PIL import Image
        return np.asarray(Image.open(path))
    raw = open(path, "rb").read()
    _, dims, _, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    return np.frombuffer(body, np.uint8).reshape(h, w)


def test_save_seg_preds_from_a_device_store(dev, tmp_path):
    gt, probs, store, _ = _session(dev, np.random.default_rng(21))
    meta = dict(sequence="seq", n_interaction=1, scribble_iter=2)
    paths = misc.save_seg_preds(store.all_P, meta, str(tmp_path / "a"))
    want = R.quantize_probs(probs, 3)
    assert len(paths) == 3 * 4 and paths[0].endswith(os.path.join("interaction-1", "scribble-2", "seq", "probs", "1", "00000" + paths[0][-4:]))
    for k, p in enumerate(paths):
        np.testing.assert_array_equal(_read_gray(p), want[k // 4, k % 4], err_msg=p)
    again = misc.save_seg_preds(store, meta, str(tmp_path / "b"))         # the store itself, and the reference layout on the host
    host = misc.save_seg_preds(probs, meta, str(tmp_path / "c"))
    for a, b, c in zip(paths, again, host):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


@pytest.mark.parametrize("metric", ["J_AND_F", "J"])
def test_assess_report_equals_the_steps_and_a_captured_graph(lib, dev, metric):
    rng = np.random.default_rng(31)
    gt, probs, store, scores = _session(dev, rng)
    gt2, probs2, store2, scores2 = _session(dev, rng, n=2, H=9, W=16, O=1)
    gtd, gtd2 = torch.from_numpy(gt).to(dev), torch.from_numpy(gt2).to(dev)
    rep, res = utils_agent.assess_report([(gtd, store, 3), (gtd2, store2.all_P, 1)], [scores, scores2], metric)
    assert rep.shape == (2, 3) and rep.dtype == np.float32
    # step by step, against the restatement and the oracle-checked count pass
    planes = [metrics.quantize_probs(store, 3), metrics.quantize_probs(store2, 1)]
    np.testing.assert_array_equal(planes[0].cpu().numpy(), R.quantize_probs(probs, 3))
    counts, lengths, n_obj = metrics.qa_counts([(gtd, planes[0], 3), (gtd2, planes[1], 1)])
    assert (lengths, n_obj) == ([4, 2], [3, 1])
    assert torch.equal(counts, res.counts)
    c = counts.cpu().numpy()
    cs = [c[:4 * 3 * 6].reshape(4, 3, 6), c[4 * 3 * 6:].reshape(2, 1, 6)]
    for cv, g, pl, ids in ((cs[0], gt, planes[0], [1, 2, 3]), (cs[1], gt2, planes[1], [1])):
        v = _Vid(dev, g, pl.cpu().numpy(), ids)
        _assert_oracle(v, cv)
    off = 0
    for k, (cv, sc) in enumerate(zip(cs, (scores, scores2))):
        t, v = R.unit_targets(cv, metric)
        assert res.views[k].cpu().numpy().tobytes() == t.reshape(res.views[k].shape).tobytes()
        np.testing.assert_array_equal(res.valid_views[k].cpu().numpy().reshape(-1), v)
        wl, wd, wn = R.reference_loop(sc.cpu().numpy().reshape(-1), t, v)
        assert (rep[k, 0].tobytes(), rep[k, 1].tobytes(), int(rep[k, 2])) == (wl.tobytes(), wd.tobytes(), wn)
        off += t.size
    assert 0 < int(rep[0, 2]) <= 12 and 0 < int(rep[1, 2]) <= 2
    # one captured graph of quantise, counts and targets, replayed twice, equals the eager result
    flat = torch.cat([scores.reshape(-1), scores2.reshape(-1)])
    gts = [gtd, gtd2]
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pl = [metrics.quantize_probs(store, 3), metrics.quantize_probs(store2, 1)]
        out = metrics.qa_targets([(gts[0], pl[0], 3), (gts[1], pl[1], 1)], metric, scores=flat)
        packed = out.report
    for _ in range(2):
        out.target.fill_(-1.0)
        packed.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert packed.cpu().numpy().tobytes() == rep.tobytes()
        assert torch.equal(out.target, res.target) and torch.equal(out.valid, res.valid)


SMALL = ["with", "synthetic=1", "setting=wild", "method=ours", "synth.n_sequences=2", "synth.n_frames=6", "synth.height=48", "synth.width=80",
         "eval_max_nb_interactions=2"]


def _strip_times(text):
    return re.sub(r"(rec_time:|recommend_frame avg |frame-cache uploads )\s*[0-9.]+", r"\1T", text)      # (the upload counter is per process)


def test_run_eval_with_and_without_the_keys(dev, tmp_path, capsys):
    from ivos_w_amd import entry
    common = SMALL + [f"ckpt_dir={tmp_path}/weights"]
    outs, texts = {}, {}
    for name, extra, drop in (("keys", ["qa_report=true", "save_probs=true", f"agent.save_result_dir={tmp_path}/train"], False),
                              ("off", ["qa_report=false", "save_probs=false"], False), ("absent", [], True)):
        cfg = entry.parse_cli(common + extra + [f"report_save_dir={tmp_path}/{name}"])
        if drop:
            del cfg["qa_report"], cfg["save_probs"]
        utils_agent.clear_frame_cache()
        torch.manual_seed(0)
        outs[name] = entry.run_eval(cfg, "MANet")
        texts[name] = capsys.readouterr().out
        assert utils_agent.score_tap is None
    on = json.load(open(os.path.join(outs["keys"]["report_dir"], "summary.json")))
    qa = on["qa"]
    assert set(qa) == {"loss", "diff", "valid", "units"} and 0 < qa["valid"] <= qa["units"] and qa["loss"] >= 0 and qa["diff"] >= 0
    lines = [ln for ln in texts["keys"].splitlines() if ln.startswith("avg_")]
    assert len(lines) == 4 and all(re.search(r"corr: \S+ qa_loss: [0-9.]+ qa_diff: [0-9.]+ valid: \d+/\d+ seq:", ln) for ln in lines)
    assert "save_probs=true" in texts["keys"]
    root = os.path.join(str(tmp_path), "train")
    files = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    assert files and all(re.fullmatch(r"interaction-[12]/scribble-1/[^/]+/probs/[1-9]/0000[0-5]\.(png|pgm)", f.replace(os.sep, "/")) for f in files)
    assert len(files) == qa["units"] and qa["units"] % 6 == 0              # one file per (interaction, object, frame) unit
    # without the keys: no file, no "qa", and stdout / summary.json are those of a run that never heard of them
    raw = {k: open(os.path.join(outs[k]["report_dir"], "summary.json"), "rb").read() for k in ("off", "absent")}
    assert raw["off"] == raw["absent"] and set(json.loads(raw["off"])) == {"auc", "curve"}
    strip = lambda k: _strip_times(texts[k]).replace(f"{tmp_path}/{k}", "DIR")
    assert strip("off") == strip("absent") and "qa_" not in texts["off"] and "save_probs" not in texts["off"]
    assert json.loads(raw["off"]) == {k: v for k, v in on.items() if k != "qa"}      # the keys change nothing else
    assert [re.sub(r"qa_loss.*valid: \d+/\d+ ", "", _strip_times(ln)) for ln in lines] == \
        [_strip_times(ln) for ln in texts["off"].splitlines() if ln.startswith("avg_")]


def test_generate_data_writes_the_planes_of_two_interactions(dev, tmp_path, capsys):
    """generate_data.py's entry: the synthetic loop with save_probs=true fixed; the files equal the restatement of the session's all_P."""
    from ivos_w_amd import entry
    seen = []
    real = misc.save_seg_preds

    def spy(probs, meta, out_dir):
        paths = real(probs, meta, out_dir)
        seen.append((dict(meta), paths, probs.cpu().numpy().copy()))
        return paths
    misc.save_seg_preds = spy
    try:
        utils_agent.clear_frame_cache()
        out = entry.main_generate(SMALL[:1] + ["setting=oracle", "method=ours"] + SMALL[4:] +
                                  [f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/gen", f"agent.save_result_dir={tmp_path}/samples"])
    finally:
        misc.save_seg_preds = real
    text = capsys.readouterr().out
    assert "generate_data: the synthetic back end" in text and f"save_probs=true -> {tmp_path}/samples" in text
    assert "qa" not in json.load(open(os.path.join(out["report_dir"], "summary.json")))
    assert len(seen) == 4 and [m["n_interaction"] for m, _, _ in seen] == [1, 2, 1, 2]
    n_files = 0
    for meta, paths, planes in seen:
        assert planes.dtype == np.uint8 and planes.shape[1:] == (6, 48, 80) and len(paths) == planes.shape[0] * 6
        assert paths[0].startswith(os.path.join(str(tmp_path), "samples", f"interaction-{meta['n_interaction']}", "scribble-1", meta["sequence"], "probs", "1", "00000"))
        for k, p in enumerate(paths):
            np.testing.assert_array_equal(_read_gray(p), planes[k // 6, k % 6], err_msg=p)
            n_files += 1
        assert planes.max() >= 205 and planes.min() < 205
    assert n_files == sum(len(fs) for _, _, fs in os.walk(os.path.join(str(tmp_path), "samples")))
