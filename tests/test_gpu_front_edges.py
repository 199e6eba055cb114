"""The kernels around the conv tower at their edges, each against a float64 reference (oracle/front_ref.py, pinned on the CPU
by tests/test_oracle_front.py), through the C ABI:

  a. ivosw_mask_bbox         bit-exact on the float4 scan and, from a misaligned base, the scalar scan: chunk seams, B > 2048, the
                             0.5 threshold, and the (y, x) carried over several 1024-element strides at W < 4, W < 1024,
                             W = 1024 and W > 1024 (the B = 1 and B = 2049 tests; the 14-size batches carry only at 480 x 854)
  b. ivosw_roi_sample(_u8)   inside an error bound derived from the sample point's float32 roundings, on ramps (where the value
                             IS the coordinate) and on a random image
  c. ivosw_quality_state     bit-exact against numpy's float64 pairwise mean at every branch of the reduction
  d. pool + fc1              against float64 on the kernel's own res5 tap, in the error class of torch's float32
  e. forward_objects         equal to forward on materialised copies, also from mask planes at odd strides
"""
import functools

import numpy as np
import pytest
import torch

from ivos_w_amd import synth
from ivos_w_amd import _lib as L
from oracle import front_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- a. mask -> box
def _misaligned(t):
    """The same values in a buffer that starts 4 bytes behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4
    return v


def _bbox(dev, d_tp, B, H, W):
    out = torch.empty(B, 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(B, 4, dtype=torch.int32, device=dev)
    L.check(L.lib().ivosw_mask_bbox(L.dptr(d_tp), B, H, W, L.dptr(out), L.dptr(scratch), L.stream_ptr(dev)), "mask_bbox")
    return out.cpu().numpy(), scratch.cpu().numpy()


def _assert_bbox(dev, d_tp, tp, why):
    """(y,x,h,w) equal to bbox_ref, and the integer min / max the scan left in the scratch equal to bbox_minmax_ref (on small
    frames every box is clamped to the whole frame: only the integers see a wrong coordinate there)."""
    B, H, W = tp.shape
    yxhw, raw = _bbox(dev, d_tp, B, H, W)
    np.testing.assert_array_equal(yxhw, fr.bbox_ref(tp), err_msg=why)
    np.testing.assert_array_equal(raw, fr.bbox_minmax_ref(tp), err_msg=why + ": integer box in the scratch")


@pytest.mark.parametrize("H,W", fr.BBOX_SIZES)
def test_bbox_is_exact_on_every_scan_path(dev, H, W):
    """The float4 scan from a 16-byte aligned base (where H * W % 4 == 0) and the scalar scan from a base 4 bytes later, on the
    planes of fr.bbox_planes.  Except at 480 x 854 a workgroup's chunk is one 1024-element stride here: the start (y, x) comes from
    the division and nothing is carried - the carried coordinates at other widths are the business of the two tests below."""
    tp, seams = fr.bbox_planes(H, W)
    B = tp.shape[0]
    assert fr.scan_seams(B, H, W) == seams and (len(seams) > 0) == (H * W > 1024)
    d = torch.from_numpy(tp).to(dev)
    assert d.data_ptr() % 16 == 0
    _assert_bbox(dev, d, tp, "16-byte aligned base")
    _assert_bbox(dev, _misaligned(d), tp, "base + 4 bytes (scalar scan)")


# One chunk per sample (B > 2048: S = 1): the whole plane is ONE workgroup's range, so at planes above 1024 elements the float4 scan
# walks several 1024-element strides and every visit after the first uses the CARRIED (y, x): sy = 0, sx = 1024 at W = 1100 and 1025
# (a wrap every stride or so), sy = 1, sx = 0 at W = 1024, sy = 512, sx = 0 at W = 2 (a float4 spans two rows).  4 x 1024 and 2048 x 2
# run the four-loads-in-flight loop for every lane, 4 x 1025 and 4 x 1100 run it and the single-load tail.
@pytest.mark.parametrize("H,W", [(8, 8), (4, 1025), (4, 1024), (4, 1100), (2048, 2)])
def test_bbox_one_chunk_per_sample(dev, H, W):
    """B = 2049: grid (1, B).  A lone pixel on each side of every 1024-element stride (and at the plane's and rows' ends), one
    plane each; full, empty and sparse planes in the other slots."""
    B = 2049
    rs = np.random.RandomState(2049 + W)
    tp = np.where(rs.rand(B, H, W) < 2.0 / (H * W), 0.9, 0.1 * rs.rand(B, H, W)).astype(np.float32)
    pos = fr.stride_edges(H, W)
    assert len(pos) + 1 < B and (H * W <= 1024 or {1023, 1024, 1027} <= set(pos))
    tp[0] = 1.0
    for k, p in enumerate(pos):                  # the last samples of the batch included
        b = B - 1 - k
        tp[b] = 0.0
        tp[b].reshape(-1)[p] = 1.0
    assert fr.scan_seams(B, H, W) == []
    assert len(np.unique(fr.bbox_minmax_ref(tp), axis=0)) > 100
    d = torch.from_numpy(tp).to(dev)
    assert d.data_ptr() % 16 == 0
    _assert_bbox(dev, d, tp, "16-byte aligned base")
    _assert_bbox(dev, _misaligned(d), tp, "base + 4 bytes (scalar scan)")


@pytest.mark.parametrize("H,W", [(480, 854), (70, 1100), (80, 1024)])
def test_bbox_single_sample_at_full_width_of_the_scan(dev, H, W):
    """B = 1: S = 64 requested.  480 x 854: 58 chunks of 7168 (seven strides each, W < 1024) - a lone pixel on each side of every
    seam.  70 x 1100 and 80 x 1024: chunks of 2048, two strides per workgroup with the second visit at the carried (y, x), W > 1024
    (sy = 0) and W = 1024 (sx = 0) - a lone pixel on each side of every seam AND of every stride.  Plus the plane's ends and a
    sparse plane; from a 16-byte aligned base (float4 scan) and 4 bytes later (scalar scan)."""
    seams = fr.scan_seams(1, H, W)
    assert len(seams) == {854: 57, 1100: 37, 1024: 39}[W] and seams[0] == {854: 7168, 1100: 2048, 1024: 2048}[W]
    pos = sorted({p for s in seams for p in (s - 1, s)} | {H * W - 1, H * W - 4, 0} | (set(fr.stride_edges(H, W)) if W >= 1024 else set()))
    yx = np.array([[p // W, p // W, p % W, p % W] for p in pos], np.int32)
    sparse = fr.sparse_plane(np.random.RandomState(1), H, W)[None]
    want_raw = np.concatenate([yx, fr.bbox_minmax_ref(sparse)])
    plane, want = np.zeros((1, H, W), np.float32), np.zeros((len(pos) + 1, 4), np.float32)
    for i, p in enumerate(pos):
        plane.reshape(-1)[p] = 1
        want[i] = fr.bbox_ref(plane)[0]
        plane.reshape(-1)[p] = 0
    want[-1] = fr.bbox_ref(sparse)[0]
    for mis in (0, 1):
        d = torch.zeros(H * W + 4, dtype=torch.float32, device=dev)[mis:mis + H * W]
        assert d.data_ptr() % 16 == 4 * mis
        out = torch.empty(len(pos) + 1, 4, dtype=torch.float32, device=dev)
        scratch = torch.empty(len(pos) + 1, 4, dtype=torch.int32, device=dev)
        for i, p in enumerate(pos):
            d[p] = 1.0
            L.check(L.lib().ivosw_mask_bbox(L.dptr(d), 1, H, W, L.dptr(out[i:i + 1]), L.dptr(scratch[i:i + 1]), L.stream_ptr(dev)), "mask_bbox")
            d[p] = 0.0
        d.copy_(torch.from_numpy(sparse.reshape(-1)).to(dev))
        L.check(L.lib().ivosw_mask_bbox(L.dptr(d), 1, H, W, L.dptr(out[-1:]), L.dptr(scratch[-1:]), L.stream_ptr(dev)), "mask_bbox")
        np.testing.assert_array_equal(scratch.cpu().numpy(), want_raw, err_msg=f"misaligned={mis}: integer box in the scratch")
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"misaligned={mis}")


# ---------------------------------------------------------------- b. ROI sampler coordinates
@functools.lru_cache(maxsize=None)
def _roi_case(kind, H, W, u8):
    return fr.roi_case(kind, H, W, u8)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("kind", fr.ROI_KINDS)
@pytest.mark.parametrize("H,W", fr.ROI_SIZES)
def test_roi_sample_points_against_fp64(dev, capsys, H, W, kind, u8):
    """Every output value within fr.roi_bound of roi_sample64 (bound and derivation there; it is proven wide enough for a correct
    float32 sampler by tests/test_oracle_front.py), once with the slopes of the zero-padded image over every pixel and once with
    the interior slopes over the pixels whose float64 sample point lies in [1, W-2] x [1, H-2]: on a ramp the latter allows
    ~ 12 * 2^-24 on the P channel, which a sample point off by more than ~ 12 * 2^-24 * (W - 1) pixel exceeds - about 6e-4 pixel at
    480 x 854 and 4e-5 pixel at 37 x 53 (the bound grows with the frame; 2 x 2 has no interior point).  fp32 and bf16 output."""
    case = _roi_case(kind, H, W, u8)
    B = len(case["boxes"])
    d_box = torch.from_numpy(case["boxes"]).to(dev)
    d_tp = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(case["p"], (B, H, W)))).to(dev)
    if u8:
        rgbx = np.zeros((B, H, W, 4), np.uint8)
        rgbx[..., :3] = case["col"].transpose(1, 2, 0)[None]
        d_tf, fn, what = torch.from_numpy(rgbx).to(dev), L.lib().ivosw_roi_sample_u8, "roi_sample_u8"
    else:
        d_tf = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(case["col"], (B, 3, H, W)))).to(dev)
        fn, what = L.lib().ivosw_roi_sample, "roi_sample"
    ratios = {}
    for name, code, tdt in (("fp32", L.F32, torch.float32), ("bf16", L.BF16, torch.bfloat16)):
        roi = torch.empty(B, 256, 256, 4, device=dev, dtype=tdt)
        L.check(fn(L.dptr(d_tf), L.dptr(d_tp), L.dptr(d_box), B, H, W, code, L.dptr(roi), L.stream_ptr(dev)), what)
        ratios[name] = fr.roi_check(roi.float().cpu().numpy(), case, H, W, bf16=(name == "bf16"))
    with capsys.disabled():
        print(f"\n[roi vs fp64] {H}x{W} {kind} {'u8' if u8 else 'f32'}: error / bound fp32 {ratios['fp32'][0]:.3f} (all) {ratios['fp32'][1]:.3f} (interior), "
              f"bf16 {ratios['bf16'][0]:.3f} (all) {ratios['bf16'][1]:.3f} (interior)")
    for name, (worst_all, worst_in) in ratios.items():
        assert worst_all <= 1.0, (name, "every pixel", worst_all)
        assert worst_in <= 1.0, (name, "interior", worst_in)


# ---------------------------------------------------------------- c. quality / state
@pytest.mark.parametrize("n_frames", fr.QUALITY_N_FRAMES)
@pytest.mark.parametrize("n_obj", fr.QUALITY_N_OBJ)
def test_quality_state_is_numpys_float64_mean(dev, n_obj, n_frames):
    """Bit-exact on magnitudes 1e-3 .. 1e3 (the specified range, on which any summation order is exact in float64) and on
    1e-7 .. 1e7, where the order shows (tests/test_oracle_front.py::test_quality_inputs_discriminate)."""
    for dec in fr.QUALITY_DECADES:
        scores, counts = fr.quality_inputs(n_obj, n_frames, dec)
        want_q = fr.quality_ref(scores)
        want_s = np.stack([want_q.astype(np.float32), counts], 1)
        d_sc, d_cnt = torch.from_numpy(scores).to(dev), torch.from_numpy(counts).to(dev)
        q = torch.full((n_frames,), float("nan"), dtype=torch.float64, device=dev)
        st = torch.full((n_frames, 2), float("nan"), dtype=torch.float32, device=dev)
        L.check(L.lib().ivosw_quality_state(L.dptr(d_sc), n_obj, n_frames, L.dptr(d_cnt), L.dptr(q), L.dptr(st), L.stream_ptr(dev)),
                "quality_state")
        np.testing.assert_array_equal(q.cpu().numpy(), want_q, err_msg=f"quality, decades {dec}")
        np.testing.assert_array_equal(st.cpu().numpy(), want_s, err_msg=f"state, decades {dec}")


# ---------------------------------------------------------------- d. head, e. indirection
def _net(dev, precision):
    from ivos_w_amd.models.assessment import AssessNet
    net = AssessNet(precision=precision)
    sd = synth.assessnet_state_dict(0, spread=True)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def nets(dev):
    return {"fp32": _net(dev, "fp32"), "bf16": _net(dev, "bf16")}


def _video(n, C, H, W, seed):
    """n frames [n,3,H,W] and C mask planes per frame [n,C,H,W]: soft rectangles (0.9 on 0.1), another one per plane."""
    rs = np.random.RandomState(seed)
    tf = rs.rand(n, 3, H, W).astype(np.float32)
    tp = (0.1 * rs.rand(n, C, H, W)).astype(np.float32)
    for i in range(n):
        for c in range(C):
            y0, x0 = rs.randint(0, H // 2), rs.randint(0, W // 2)
            tp[i, c, y0:y0 + rs.randint(3, H // 2), x0:x0 + rs.randint(3, W // 2)] = 0.9
    return tf, tp


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_head_against_fp64_is_in_the_class_of_torch_fp32(dev, nets, capsys, precision):
    """pooled and scores against head_ref (float64) of the res5 tap the kernel itself produced.  Yardstick: torch's float32
    avg_pool2d + linear on the CPU on the same tap, measured against the same float64 values, relative to the tensor's largest
    value.  Bar (as test_bptt_error_against_fp64_is_in_the_class_of_torch_fp32): HIP error <= 2 x torch's, or <= 1e-6 of the scale."""
    import torch.nn.functional as F
    net = nets[precision]
    tf, tp = _video(3, 1, 64, 64, seed=64)
    ttf, ttp = torch.from_numpy(tf).to(dev), torch.from_numpy(tp[:, 0]).to(dev)
    s5, res5 = net.forward_tap(ttf, ttp, "res5")
    sp, pooled = net.forward_tap(ttf, ttp, "pooled")
    assert torch.equal(s5, sp) and torch.equal(sp.reshape(-1), net(ttf, ttp).reshape(-1))
    assert res5.dtype == (torch.float32 if precision == "fp32" else torch.bfloat16) and tuple(res5.shape) == (3, 8, 8, 2048)
    x32 = res5.float().cpu()
    sd = synth.assessnet_state_dict(0, spread=True)
    fw, fb = np.asarray(sd["fc1.weight"], np.float32), np.asarray(sd["fc1.bias"], np.float32)
    want_p, want_s = fr.head_ref(x32.numpy(), fw, fb)
    t_p = F.avg_pool2d(x32.permute(0, 3, 1, 2).contiguous(), 8).flatten(1)
    t_s = F.linear(t_p, torch.from_numpy(fw), torch.from_numpy(fb))[:, 0]
    rows = []
    for name, got, yard, want in (("pooled", pooled.cpu().numpy(), t_p.numpy(), want_p), ("scores", sp.reshape(-1).cpu().numpy(), t_s.numpy(), want_s)):
        scale = np.abs(want).max()
        e_hip = np.abs(got.astype(np.float64) - want).max() / scale
        e_t = np.abs(yard.astype(np.float64) - want).max() / scale
        rows.append((name, e_hip, e_t))
    with capsys.disabled():
        print(f"\n[head vs fp64] {precision}: " + ", ".join(f"{n} HIP {a:.2e} torch-fp32 {b:.2e}" for n, a, b in rows))
    for name, e_hip, e_t in rows:
        assert e_hip <= max(2 * e_t, 1e-6), (name, e_hip, e_t)


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (150, 200)])
def test_forward_objects_equals_forward_on_materialised_copies(dev, nets, H, W):
    """n = 3 frames, O = 2 objects: the frame and mask indirection of forward_objects (unit = object * n + frame over one copy of
    the frames, mask planes read in place) against forward on the frames repeated O times and contiguous copies of the planes -
    equal bits in fp32 and in bf16; and from a mask tensor whose object stride (plane + 1 elements) is odd and whose first mask
    plane starts 8 or 12 bytes behind a 16-byte boundary (scalar scan, unaligned planes in the sampler) the scores do not move.  At 37 x 53 and 64 x 64 every box is
    the whole frame (minimum extent 128, clamped), so the masks reach the scores through the sampler only; at 150 x 200 the boxes
    differ from unit to unit and the scan's indirection shows too."""
    n, O = 3, 2
    tf, tp = _video(n, O + 1, H, W, seed=H * W)
    all_F, all_P = torch.from_numpy(tf).to(dev), torch.from_numpy(tp).to(dev)
    mat_f = all_F.repeat(O, 1, 1, 1).contiguous()
    mat_p = torch.cat([all_P[:, o + 1] for o in range(O)], 0).contiguous()
    plane = H * W
    buf = torch.zeros(1 + n * (O + 1) * (plane + 1) + 4, dtype=torch.float32, device=dev)
    odd = buf[1:1 + n * (O + 1) * (plane + 1)].view(n, O + 1, plane + 1)[:, :, :plane].unflatten(2, (H, W))
    odd.copy_(all_P)
    assert odd.stride(3) == 1 and odd.stride(2) == W and odd.stride(1) == plane + 1 and odd.stride(0) == (O + 1) * (plane + 1)
    assert (odd.stride(1) % 4 != 0 or odd.stride(0) % 4 != 0) and odd[:, 1:].data_ptr() % 16 != 0
    for precision in ("fp32", "bf16"):
        net = nets[precision]
        want = net(mat_f, mat_p).reshape(O, n).clone()
        got = net.forward_objects(all_F, all_P, O).clone()
        assert torch.equal(got, want), (precision, got, want)
        got_odd = net.forward_objects(all_F, odd, O).clone()
        assert torch.equal(got_odd, want), (precision, "odd strides", got_odd, want)
        assert len(torch.unique(want)) == O * n
