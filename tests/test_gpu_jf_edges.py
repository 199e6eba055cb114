"""GPU: the DAVIS J / F kernels (csrc/metrics.hip) on the inputs of oracle/jf_cases.py - object pixels on every frame border, edges
on the 1024-pixel segment seam, the end of the buffer, ids over the whole byte range, 32 objects, dense maps, every radius at the
disk's rim, a reused workspace.  The reference is oracle/jf_oracle.py (pinned at these edges by tests/test_oracle_jf_cases.py);
everything is integer counts and float64 ratios formed by the same expressions: the bar is EQUALITY, no tolerance anywhere."""
import numpy as np
import pytest
import torch

from ivos_w_amd import metrics
from ivos_w_amd import _lib as L
from oracle import jf_cases as jc
from oracle import jf_oracle as jo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _assert_equals_oracle(c, cheap=True):
    """Counts, J and F of ivos_w_amd.metrics equal to the oracle's.  cheap: J / F straight from jo.batched_*; otherwise (dilation by a
    large disk) from the oracle's counts through jc.j_and_f, which the CPU test shows to be the same numbers."""
    ids, got = metrics.jf_counts(c.gt, c.pred, c.nb_objects, c.bound_th)
    np.testing.assert_array_equal(ids, jo._object_ids(c.gt.astype(np.int64), c.nb_objects))
    r = int(jo.bound_pixels(c.gt.shape[1:], c.bound_th))
    want = jc.counts(c.gt, c.pred, ids, r)
    bad = np.argwhere((got != want).any(axis=2))
    assert got.shape == want.shape and len(bad) == 0, \
        f"(frame, object index) {bad[:8].tolist()}: got {got[tuple(bad[0])].tolist()} want {want[tuple(bad[0])].tolist()}"
    if cheap:
        want_j = jo.batched_jaccard(c.gt, c.pred, False, c.nb_objects)
        want_f = jo.batched_f_measure(c.gt, c.pred, False, c.nb_objects, c.bound_th)
    else:
        want_j, want_f = jc.j_and_f(want)
    j, f = metrics.batched_j_and_f(c.gt, c.pred, False, c.nb_objects, c.bound_th)
    np.testing.assert_array_equal(j, want_j)
    np.testing.assert_array_equal(f, want_f)
    np.testing.assert_array_equal(metrics.batched_jaccard(c.gt, c.pred, True, c.nb_objects), want_j.mean(axis=1))
    np.testing.assert_array_equal(metrics.batched_f_measure(c.gt, c.pred, True, c.nb_objects, c.bound_th), want_f.mean(axis=1))


@pytest.mark.parametrize("H,W,r", jc.BORDER_SHAPES)
def test_objects_on_the_frame_borders(dev, H, W, r):
    _assert_equals_oracle(jc.border_case(H, W, r))


@pytest.mark.parametrize("H,W", jc.SEAM_SHAPES)
def test_edges_on_the_segment_seam(dev, H, W):
    _assert_equals_oracle(jc.seam_case(H, W))


@pytest.mark.parametrize("N,H,W", jc.TAIL_SHAPES)
def test_end_of_the_buffer_and_the_bytes_behind_a_row(dev, N, H, W):
    _assert_equals_oracle(jc.tail_case(N, H, W))


def test_ids_over_the_byte_range(dev):
    _assert_equals_oracle(jc.iid_bytes_case())           # labels iid over 0..255, ids 1..32
    _assert_equals_oracle(jc.unique_ids_case())          # ids {1, 7, 127, 128, 200, 254} from the labels, 255 = void
    _assert_equals_oracle(jc.many_objects_case())        # 32 objects


def _cabi_counts(dev, gt, pred, ids, r):
    N, H, W = gt.shape
    lib = L.lib()
    d_gt, d_pr = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    out = torch.full((N, len(ids), 6), -1, dtype=torch.int64, device=dev)
    nbytes = lib.ivosw_jf_ws_bytes(N, H, W, len(ids))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    rc = lib.ivosw_jf_counts(L.dptr(d_gt), L.dptr(d_pr), N, H, W, bytes(ids), len(ids), r, L.dptr(out), L.dptr(ws), nbytes, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy()


def test_c_abi_id_list_in_any_order(dev):
    """An id list that is not ascending and holds 0, 255 and ids on both sides of 128: at the C ABI an id is a byte to compare with."""
    c = jc.iid_bytes_case()
    ids = list(jc.CABI_IDS)
    rc, got = _cabi_counts(dev, c.gt, c.pred, ids, 2)
    assert rc == 0
    np.testing.assert_array_equal(got, jc.counts(c.gt, c.pred, ids, 2))
    u = jc.unique_ids_case()
    rc, got = _cabi_counts(dev, u.gt, u.pred, ids, 1)
    assert rc == 0
    np.testing.assert_array_equal(got, jc.counts(u.gt, u.pred, ids, 1))


def test_c_abi_refuses_what_the_grid_cannot_hold(dev):
    """33 objects, and N * n_obj = 65536 at H = W = 1: IVOSW_ERR_ARG (-1) and nothing launched - the counts keep their fill value."""
    g = np.ones((2, 1, 1), np.uint8)
    rc, out = _cabi_counts(dev, g, g, list(range(1, 34)), 1)
    assert rc == -1 and (out == -1).all() and b"32" in L.lib().ivosw_last_error()
    g = np.ones((2048, 1, 1), np.uint8)
    rc, out = _cabi_counts(dev, g, g, list(range(1, 33)), 1)
    assert rc == -1 and (out == -1).all() and b"65535" in L.lib().ivosw_last_error()
    g = np.ones((2047, 1, 1), np.uint8)                  # 65504 <= 65535: the largest multiple of 32 that is accepted
    rc, out = _cabi_counts(dev, g, g, list(range(1, 33)), 1)
    assert rc == 0
    np.testing.assert_array_equal(out[:, 0], np.tile([1, 1, 0, 0, 0, 0], (2047, 1)))
    assert (out[:, 1:] == 0).all()
    with pytest.raises(RuntimeError):
        metrics.jf_counts(np.ones((1, 2, 2), np.uint8), np.ones((1, 2, 2), np.uint8), nb_objects=33)


def test_dense_maps_and_full_counters(dev):
    _assert_equals_oracle(jc.checkerboard_case())
    _assert_equals_oracle(jc.coin_flip_case())
    for c in jc.full_wave_case():                        # 4096 intersection and 4096 union pixels in every wave
        _assert_equals_oracle(c)


@pytest.mark.parametrize("r,part", [(r, p) for r in jc.RADII for p in jc.RADIUS_PARTS if not (r == 0 and p == "rim")])
def test_every_radius_at_the_disks_rim(dev, r, part):
    _assert_equals_oracle(jc.radius_case(r, part), cheap=r < 16)


def test_small_call_after_a_large_one_reads_no_stale_words(dev):
    big, small = jc.reuse_cases()
    _assert_equals_oracle(big)
    ws = metrics._ws[(dev.index, "jf")]
    before = ws.data_ptr()
    assert ws.numel() >= 2 * 3 * 4 * 64 * 10 * 4
    _assert_equals_oracle(small)
    assert metrics._ws[(dev.index, "jf")].data_ptr() == before        # the same, larger buffer served the small call
