"""Pins oracle/front_ref.py (the float64 references of tests/test_gpu_front_edges.py) on the CPU: against the fp32 oracle and
the goldens it is pinned to, against torch in float64, and - before any kernel meets them - that the ROI error bound is not too
tight for a correct fp32 sampler and that the quality inputs can tell numpy's summation order from a sequential one."""
import numpy as np
import pytest
import torch

from ivos_w_amd import synth
from oracle import assess_oracle as ao
from oracle import front_ref as fr


@pytest.mark.parametrize("B,edge", [(8, True), (1, False), (3, False)])
def test_bbox_ref_is_the_oracle_bbox_on_the_golden_inputs(B, edge):
    _, tp = synth.assess_inputs(B, seed=1234 + B, edge_cases=edge, structured=True)
    np.testing.assert_array_equal(fr.bbox_ref(tp), ao.mask_bbox_yxhw((tp > 0.5).astype(np.float32), 1.5))


def test_bbox_ref_threshold_and_nan():
    half = np.float32(0.5)
    vals = np.array([half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), 0.49, -1, np.nan, np.inf], np.float32)
    tp = np.zeros((len(vals), 200, 300), np.float32)
    for b, v in enumerate(vals):
        tp[b, 150, 20] = v
    got = fr.bbox_ref(tp)
    empty, one = fr.bbox_ref(np.zeros((1, 200, 300), np.float32))[0], fr.bbox_ref((np.arange(60000) == 150 * 300 + 20).reshape(1, 200, 300))[0]
    assert not np.array_equal(empty, one)
    for b, fg in enumerate([False, True, False, False, False, False, True]):
        np.testing.assert_array_equal(got[b], one if fg else empty, err_msg=str(vals[b]))


@pytest.mark.parametrize("H,W", fr.BBOX_SIZES)
def test_bbox_planes_tell_a_wrong_threshold_and_cover_the_seams(H, W):
    """The batch of the GPU test: a scan that took 0.5 itself, or NaN, for foreground would leave other integers than
    bbox_minmax_ref at every size; every seam of the batch's own size has a lone pixel on each side; and the (y,x,h,w) rows follow
    from the integers by the oracle's rule."""
    tp, seams = fr.bbox_planes(H, W)
    raw = fr.bbox_minmax_ref(tp)
    with np.errstate(invalid="ignore"):
        ge = fr.bbox_minmax_ref(np.where(tp >= np.float32(0.5), 1, 0))
        nan_fg = fr.bbox_minmax_ref(np.where(tp <= np.float32(0.5), 0, 1))
    assert (raw != ge).any() and (raw != nan_fg).any()
    assert seams == fr.scan_seams(tp.shape[0], H, W)
    lone = {(int(r[0]) * W + int(r[2])) for r in raw if r[0] == r[1] and r[2] == r[3]}
    assert all(s - 1 in lone and s in lone for s in seams) and H * W - 1 in lone
    np.testing.assert_array_equal(fr.bbox_ref(tp), ao.mask_bbox_yxhw((tp > 0.5).astype(np.float32), 1.5))


def test_scan_seams_rule():
    assert fr.scan_seams(1, 480, 854) == list(range(7168, 409920, 7168))           # S = 64: ceil(409920 / 64) = 6405 -> 7168, 58 chunks
    assert fr.scan_seams(2049, 8, 8) == [] and fr.scan_seams(40, 37, 53) == [1024]
    assert fr.scan_seams(100, 3, 1100) == [1024, 2048, 3072]                        # S = 20: 165 -> 1024
    assert fr.scan_seams(4096, 3, 1100) == []                                        # B > 2048: S = 1, one chunk per sample


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("kind", fr.ROI_KINDS)
@pytest.mark.parametrize("H,W", fr.ROI_SIZES)
def test_roi_bound_holds_for_the_fp32_oracle(H, W, kind, u8):
    """assess_oracle.roi_sample (float32, pinned to the reference's grid_sample by the goldens) stays inside roi_bound around
    roi_sample64 on every case the GPU test runs: the bound is not too tight for a correct float32 sampler."""
    case = fr.roi_case(kind, H, W, u8)
    B = len(case["boxes"])
    got = ao.roi_sample(np.broadcast_to(case["img"], (B,) + case["img"].shape), ao.roi_theta(case["boxes"], H, W)).astype(np.float32)
    got[:, :3] = (got[:, :3] - fr.MEAN.astype(np.float32)[None, :, None, None]) / fr.STD.astype(np.float32)[None, :, None, None]
    worst_all, worst_in = fr.roi_check(got.transpose(0, 2, 3, 1), case, H, W)
    print(f"[roi bound, fp32 oracle] {H}x{W} {kind}{' u8' if u8 else ''}: error / bound {worst_all:.3f} (all), {worst_in:.3f} (interior)")
    assert worst_all <= 1.0 and worst_in <= 1.0
    assert case["inside"].any() == (min(H, W) > 2)


def test_roi_sample64_on_integer_points_and_in_the_padding():
    """Known answers: a box whose 256 points fall on pixel centres reads the image back; half a pixel outside is half the value."""
    rs = np.random.RandomState(3)
    img = rs.rand(1, 1, 256, 256)
    np.testing.assert_allclose(fr.roi_sample64(img, np.array([[127.5, 127.5, 255.0, 255.0]], np.float32)), img, rtol=0, atol=1e-12)
    sx, sy = fr.roi_points64(np.array([[127.5, 127.0, 255.0, 255.0]], np.float32), 256, 256)
    np.testing.assert_allclose(sx[0], np.arange(256) - 0.5, atol=1e-12)
    got = fr.roi_sample64(img, np.array([[127.5, 127.0, 255.0, 255.0]], np.float32))
    np.testing.assert_allclose(got[0, 0, :, 0], 0.5 * img[0, 0, :, 0], atol=1e-12)
    assert fr.lipschitz(np.ones((3, 3))) == (1.0, 1.0) and fr.lipschitz_interior(np.ones((3, 3))) == (0.0, 0.0)


@pytest.mark.parametrize("n_obj", fr.QUALITY_N_OBJ)
def test_quality_inputs_discriminate(n_obj):
    """For n_obj >= 9 numpy sums 8 interleaved partial sums plus a tail; on the wide-magnitude inputs a sequential float64 sum of
    the same scores gives other bits on at least one frame (on EVERY n_frames > 1 of the GPU test).  Below 8 the two orders are
    the same order.  On the 10^-3 .. 10^3 inputs every order is exact (see quality_inputs): asserted too, so nobody relies on them
    for the order."""
    for n_frames in fr.QUALITY_N_FRAMES:
        for dec in fr.QUALITY_DECADES:
            scores, counts = fr.quality_inputs(n_obj, n_frames, dec)
            assert scores.dtype == np.float32 and scores.shape == (n_obj, n_frames) and counts.shape == (n_frames,)
            a = np.abs(scores)
            assert (scores < 0).any() or n_obj * n_frames < 4
            assert a.min() >= 10.0 ** -dec * 0.999 and a.max() <= 10.0 ** dec * 1.001
            differs = not np.array_equal(fr.quality_ref(scores), fr.quality_sequential(scores))
            if dec == 3 or n_obj < 8:
                assert not differs
            elif n_obj >= 9 and n_frames > 1:
                assert differs, (n_obj, n_frames)
    if n_obj >= 9:
        assert any(not np.array_equal(fr.quality_ref(s), fr.quality_sequential(s))
                   for s in (fr.quality_inputs(n_obj, n, 7)[0] for n in fr.QUALITY_N_FRAMES))


def test_quality_ref_is_numpys_pairwise_order():
    """quality_ref against the order written out: 8 interleaved partial sums, combined pairwise, then the tail."""
    for n_obj in (8, 9, 16, 17, 31):
        s = fr.quality_inputs(n_obj, 65, 7)[0].astype(np.float64)
        r = [s[j].copy() for j in range(8)]
        i = 8
        while i + 8 <= n_obj:
            for j in range(8):
                r[j] = r[j] + s[i + j]
            i += 8
        tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n_obj):
            tot = tot + s[k]
        np.testing.assert_array_equal(fr.quality_ref(s.astype(np.float32)), tot / n_obj)


def test_head_ref_is_avg_pool_plus_linear_in_float64():
    rs = np.random.RandomState(5)
    x = np.maximum(rs.standard_normal((3, 8, 8, 2048)), 0).astype(np.float32)
    w, b = rs.uniform(-0.1, 0.1, (1, 2048)).astype(np.float32), rs.uniform(-1, 1, 1).astype(np.float32)
    pooled, score = fr.head_ref(x, w, b)
    t = torch.from_numpy(x).double().permute(0, 3, 1, 2).contiguous()
    tp = torch.nn.functional.avg_pool2d(t, 8).flatten(1)
    ts = torch.nn.functional.linear(tp, torch.from_numpy(w).double(), torch.from_numpy(b).double())[:, 0]
    np.testing.assert_allclose(pooled, tp.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(score, ts.numpy(), rtol=1e-12, atol=1e-13)
