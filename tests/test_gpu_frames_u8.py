"""8-bit frames on the device: ivosw_frames_pack_u8 writes exactly the RGBX8 bytes, and every _u8 entry - the sampler, the whole forward
in the three precisions, forward_objects through the frame indirection and the two-stream split, recommend_frame - returns BIT FOR BIT
what its fp32 counterpart returns on u8.float() / 255.  No tolerance is introduced: the 8-bit path is defined as equal to the float path,
whose pins against the reference (assess_forward.npz, 1e-4 / 4e-3) stand for both."""
import ctypes

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models.assessment import AssessNet, PackedFrames, pack_frames
from ivos_w_amd.utils import utils_agent
from oracle import assess_oracle as ao

pytestmark = pytest.mark.gpu


class AD(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()}
    out = {}
    for prec in ("fp32", "bf16", "bf16x3"):
        net = AssessNet(precision=prec)
        net.load_state_dict(sd, strict=True)
        out[prec] = net.to(dev).eval()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _video(n, H, W, seed):
    """Random bytes [n,H,W,3] with 0 and 255 present, and soft blob masks [n,H,W] (one empty, one full frame when n >= 3)."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    u8[0, 0, 0, 0], u8[0, 0, 0, 1] = 0, 255
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    tp = torch.empty(n, H, W)
    for b in range(n):
        cy, cx, r = H * (0.3 + 0.4 * ((b * 7) % 5) / 5), W * (0.25 + 0.5 * ((b * 3) % 7) / 7), min(H, W) * (0.15 + 0.05 * (b % 4))
        tp[b] = torch.sigmoid((r - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) / 3.0)
    if n >= 3:
        tp[1] = 0.0
        tp[2] = 1.0
    return u8, tp


# ---------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (37, 53), (24, 44)])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_pack_equals_the_torch_permutation(dev, layout, H, W):
    """n = 2; (5,7) and (37,53) have H*W % 4 != 0: the pixels behind the last 16-byte group take the scalar path, and the CHW planes are
    not a multiple of 4 pixels, so that layout runs the per-pixel path as a whole; (2,2) is the all-vector case and (24,44) the vector path
    over more than one workgroup (528 groups of four pixels, CHW groups in both frames)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    hwc = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    src = hwc if layout == "hwc" else hwc.permute(0, 3, 1, 2).contiguous()
    want = torch.zeros(2, H, W, 4, dtype=torch.uint8)
    want[..., :3] = hwc
    for inp in (src, src.numpy(), src.to(dev)):                                # host tensor, numpy array, device tensor
        pf = pack_frames(inp, dev, layout=layout)
        assert isinstance(pf, PackedFrames) and (pf.n, pf.H, pf.W) == (2, H, W) and pf.rgbx.is_cuda and pf.rgbx.data_ptr() % 4 == 0
        assert torch.equal(pf.rgbx.cpu(), want)                                # the X byte is 0
    assert torch.equal(pf.to_float().cpu(), hwc.permute(0, 3, 1, 2).float() / 255.)
    # a source that is not 4-byte aligned (a byte-offset view) and a destination that is 4- but not 16-byte aligned: the per-pixel path
    n_src = src.numel()
    raw = torch.zeros(n_src + 16, dtype=torch.uint8, device=dev)
    raw[1:1 + n_src] = src.to(dev).reshape(-1)
    out = torch.full((2 * H * W * 4 + 16,), 0xAB, dtype=torch.uint8, device=dev)
    lib = L.lib()
    L.check(lib.ivosw_frames_pack_u8(ctypes.c_void_p(raw.data_ptr() + 1), L.U8_HWC3 if layout == "hwc" else L.U8_CHW3, 2, H, W,
                                     ctypes.c_void_p(out.data_ptr() + 4), L.stream_ptr(dev)), "frames_pack_u8")
    got = out.cpu()
    assert torch.equal(got[4:4 + 2 * H * W * 4].view(2, H, W, 4), want)
    assert bool((got[:4] == 0xAB).all()) and bool((got[4 + 2 * H * W * 4:] == 0xAB).all())        # nothing written outside the video


# ---------------------------------------------------------------------------------------------- the sampler
def _sample_both(dev, u8_hwc, tp, yxhw, dtype):
    """(8-bit sampler on the packed bytes, fp32 sampler on u8 / 255) for the same boxes."""
    lib = L.lib()
    B, H, W, _ = u8_hwc.shape
    pf = pack_frames(u8_hwc, dev)
    tf = (u8_hwc.permute(0, 3, 1, 2).float() / 255.).contiguous().to(dev)
    assert torch.equal(pf.to_float(), tf)
    d_tp, d_box = tp.contiguous().to(dev), torch.as_tensor(yxhw, dtype=torch.float32).contiguous().to(dev)
    tdt = torch.bfloat16 if dtype == L.BF16 else torch.float32
    got = torch.full((B, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
    want = torch.full((B, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
    L.check(lib.ivosw_roi_sample_u8(L.dptr(pf.rgbx), L.dptr(d_tp), L.dptr(d_box), B, H, W, dtype, L.dptr(got), L.stream_ptr(dev)), "roi_sample_u8")
    L.check(lib.ivosw_roi_sample(L.dptr(tf), L.dptr(d_tp), L.dptr(d_box), B, H, W, dtype, L.dptr(want), L.stream_ptr(dev)), "roi_sample")
    return got, want


def test_all_256_byte_values_convert_like_the_float_path(dev):
    """A 16x16 frame whose three channels each hold 0..255 (in three different orders).  Sample 0: the box of a full-frame mask;
    sample 1: the identity box, whose corner samples take one pixel with weight 1.  fp32 tile, torch.equal with the float kernel."""
    H = W = 16
    v = torch.arange(256, dtype=torch.int32).view(H, W)
    frame = torch.stack([v, 255 - v, v.t()], 2).to(torch.uint8)                # [16,16,3]
    assert all(sorted(frame[..., c].reshape(-1).tolist()) == list(range(256)) for c in range(3))
    u8 = frame[None].repeat(2, 1, 1, 1)
    tp = torch.ones(2, H, W)
    yxhw = np.stack([ao.mask_bbox_yxhw(tp[:1].numpy())[0], np.array([(H - 1) / 2, (W - 1) / 2, H - 1, W - 1], np.float32)])
    got, want = _sample_both(dev, u8, tp, yxhw, L.F32)
    assert not torch.isnan(got).any() and torch.equal(got, want)
    # the identity box really lands on pixels: its four corners are single source pixels, (v / 255 - mean) / std
    mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    g = got[1].cpu().numpy()
    for (i, j), (y, x) in (((0, 0), (0, 0)), ((0, 255), (0, 15)), ((255, 0), (15, 0)), ((255, 255), (15, 15))):
        px = frame[y, x].numpy().astype(np.float32) / np.float32(255.)
        np.testing.assert_array_equal(g[i, j, :3], (px - mean) / std)
        assert g[i, j, 3] == 1.0


EDGE_MASKS = ("empty", "corner blob of 3 pixels", "blob on the right and bottom border", "full frame")


def _edge_masks(H, W):
    tp = torch.zeros(4, H, W)
    tp[1, 0, 0] = tp[1, 0, 1] = tp[1, 1, 0] = 1.0
    tp[2, max(H - 6, 1):, max(W - 9, 1):] = 1.0
    tp[3] = 1.0
    return tp


@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", [(37, 53), (2, 2)])
def test_roi_is_bit_identical_at_the_frame_edges(dev, H, W, dtype):
    """B = 4 (empty / 3-pixel corner blob / blob on the right and bottom border / full frame), boxes from the oracle.  Frames smaller than
    the 128-pixel minimum box: the taps run off the frame on all four sides, which the test asserts from the oracle's yxhw - so it cannot
    pass without the zero-weight padding and both edge selections (x0 < 0: tap 1 takes pair.x; x0 >= W - 1: tap 0 takes pair.y)."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    u8 = torch.randint(0, 256, (4, H, W, 3), generator=g, dtype=torch.uint8)
    tp = _edge_masks(H, W)
    yxhw = ao.mask_bbox_yxhw((tp > 0.5).numpy().astype(np.float32))
    theta = ao.roi_theta(yxhw, H, W)
    lin = ao._linspace_m1_1(256)
    for b in range(4):
        sx = ((lin * theta[b, 0] + theta[b, 1] + np.float32(1)) * np.float32(0.5)) * np.float32(W - 1)
        sy = ((lin * theta[b, 2] + theta[b, 3] + np.float32(1)) * np.float32(0.5)) * np.float32(H - 1)
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        assert x0.min() < 0 and y0.min() < 0, (EDGE_MASKS[b], "left / top taps out of range")
        assert x0.max() >= W and y0.max() >= H, (EDGE_MASKS[b], "right / bottom taps out of range")
        assert (x0 == -1).any() and (x0 == W - 1).any(), (EDGE_MASKS[b], "the one-tap-in-range columns on both sides")
        assert ((x0 >= 0) & (x0 < W - 1)).any() and ((y0 >= 0) & (y0 < H - 1)).any(), (EDGE_MASKS[b], "interior taps")
    got, want = _sample_both(dev, u8, tp, yxhw, dtype)
    assert not torch.isnan(got.float()).any()
    for b in range(4):
        assert _same(got[b], want[b]), EDGE_MASKS[b]
    assert float(got.float().abs().max()) > 0.5


# ---------------------------------------------------------------------------------------------- whole forward
@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_forward_is_bit_identical_to_the_float_call(dev, nets, prec):
    net = nets[prec]
    u8, tp = _video(2, 64, 96, seed=5)
    pf, d_tp = net.pack_frames(u8), tp.to(dev)
    tf = (u8.permute(0, 3, 1, 2).float() / 255.).to(dev)
    got, want = net(pf, d_tp), net(tf, d_tp)
    assert got.shape == (2, 1) and torch.isfinite(got).all() and _same(got, want)
    s1, roi1 = net.forward_tap(pf, d_tp, "roi")
    s2, roi2 = net.forward_tap(tf, d_tp, "roi")
    assert _same(roi1, roi2) and _same(s1, s2) and _same(s1, got[:, 0])
    assert float(roi1.float().abs().max()) > 0.5


def test_a_plain_uint8_tensor_is_still_cast_unscaled(dev, nets):
    """No regression of the float path: only a PackedFrames selects the 8-bit kernels."""
    net = nets["bf16"]
    u8, tp = _video(2, 64, 96, seed=6)
    chw = u8.permute(0, 3, 1, 2).contiguous().to(dev)
    d_tp = tp.to(dev)
    a, b = net(chw, d_tp), net(chw.float(), d_tp)
    assert _same(a, b)
    assert not torch.equal(a, net(net.pack_frames(u8), d_tp))                  # 0..255 against 0..1: other scores
    with pytest.raises(AssertionError):
        net(net.pack_frames(u8), d_tp[:, :32])                                 # B, H, W are checked against the masks


# ---------------------------------------------------------------------------------------------- objects, the split
@pytest.mark.parametrize("prec,n", [("fp32", 3), ("bf16", 3), ("bf16", 33)])
def test_forward_objects_is_bit_identical_to_the_float_call(dev, nets, prec, n):
    """n = 3 frames x 2 objects; and 33 x 2 = 66 bf16 units: over the 64-unit threshold of the two-stream split, so the second half starts
    at unit u0 = 40 (object 1, frame 7) and its frame index bg % n_frames wraps."""
    net, O = nets[prec], 2
    u8, tp = _video(n, 64, 96, seed=7 + n)
    all_P = torch.zeros(n, O + 1, 64, 96)
    all_P[:, 1] = tp
    all_P[:, 2] = tp.flip(0).flip(2)
    all_P[:, 0] = 1.0 - all_P[:, 1:].amax(1)
    all_P = all_P.to(dev)
    if n == 33:
        assert L.lib().ivosw_assess_split(L.BF16, n * O, 0) == 1
    pf = net.pack_frames(u8)
    tf = pf.to_float()
    got, want = net.forward_objects(pf, all_P, O), net.forward_objects(tf, all_P, O)
    assert got.shape == (O, n) and torch.isfinite(got).all() and _same(got, want)
    assert len(set(got.reshape(-1).tolist())) > n                              # the units differ: an index mix-up could not hide


def test_recommend_frame_takes_packed_frames(dev, nets):
    from ivos_w_amd.models.agent import Agent
    net, n, O = nets["bf16"], 6, 2
    u8, tp = _video(n, 64, 96, seed=21)
    all_P = torch.zeros(n, O + 1, 64, 96)
    all_P[:, 1], all_P[:, 2] = tp, tp.flip(0)
    all_P = all_P.to(dev)
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    pf = utils_agent.pack_video(u8.numpy(), dev)
    all_F = u8.permute(0, 3, 1, 2).float() / 255.                               # the host float video the entry scripts build
    utils_agent.clear_frame_cache()
    up0 = utils_agent.frame_cache.uploads
    s_u8 = utils_agent.assess_all_objects_device(net, pf, all_P, O, dev)
    assert utils_agent.frame_cache.uploads == up0 and utils_agent.frame_cache.get(pf, dev) is pf        # handed on, never uploaded
    s_f = utils_agent.assess_all_objects_device(net, all_F, all_P, O, dev)
    assert _same(s_u8, s_f)
    np.testing.assert_array_equal(utils_agent.assess_all_objects(net, pf, all_P, O, dev), s_f.t().cpu().numpy())
    for method in ("ours", "worst"):
        picks, quals = [], []
        for frames in (pf, all_F):
            q = np.zeros(n)
            kw = dict(n_frame=n, n_objects=O, all_F=frames, all_P=all_P, new_masks_quality=np.zeros(n), prev_frames=[2],
                      annotated_frames_list=[2], mask_quality=q, first_frame=2, max_nb_interactions=8)
            picks.append(int(utils_agent.recommend_frame(AD(setting="wild", method=method), net, agent, dev, **kw)))
            quals.append(q)
        assert picks[0] == picks[1] and 0 <= picks[0] < n
        np.testing.assert_array_equal(quals[0], quals[1])
        assert np.ptp(quals[0]) > 0
    utils_agent.clear_frame_cache()


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch(dev, nets):
    lib, net = L.lib(), nets["bf16"]
    msg = lambda: lib.ivosw_last_error().decode()
    H, W = 8, 12
    u8, tp = _video(2, H, W, seed=3)
    pf, d_tp, src = net.pack_frames(u8), tp.to(dev), u8.to(dev)
    sentinel = torch.full((2, 256, 256, 4), 7.0, device=dev)
    box = torch.tensor([[4.0, 6.0, 8.0, 12.0]] * 2, device=dev)
    st = L.stream_ptr(dev)
    off = ctypes.c_void_p(pf.rgbx.data_ptr() + 1)                              # a byte-offset view of the packed video
    out = torch.full_like(pf.rgbx, 0xCD)
    assert lib.ivosw_roi_sample_u8(off, L.dptr(d_tp), L.dptr(box), 2, H, W, L.F32, L.dptr(sentinel), st) == -1 and "4-byte aligned" in msg()
    assert lib.ivosw_roi_sample_u8(None, L.dptr(d_tp), L.dptr(box), 2, H, W, L.F32, L.dptr(sentinel), st) == -1 and "null pointer" in msg()
    assert lib.ivosw_roi_sample_u8(L.dptr(pf.rgbx), L.dptr(d_tp), L.dptr(box), 2, 1, W, L.F32, L.dptr(sentinel), st) == -1 and "H, W > 1" in msg()
    assert lib.ivosw_frames_pack_u8(L.dptr(src), 2, 2, H, W, L.dptr(out), st) == -1 and "layout" in msg()
    assert lib.ivosw_frames_pack_u8(L.dptr(src), -1, 2, H, W, L.dptr(out), st) == -1 and "layout" in msg()
    assert lib.ivosw_frames_pack_u8(None, 0, 2, H, W, L.dptr(out), st) == -1 and "null pointer" in msg()
    assert lib.ivosw_frames_pack_u8(L.dptr(src), 0, 2, H, W, ctypes.c_void_p(out.data_ptr() + 2), st) == -1 and "4-byte aligned" in msg()
    packed = net._ensure_packed()
    nb = lib.ivosw_assess_ws_bytes(L.BF16, 2, H, W, 0)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    scores = torch.full((2,), 7.0, device=dev)
    fwd = lambda rgbx, hh=H: lib.ivosw_assess_forward_u8(L.dptr(packed), L.BF16, rgbx, L.dptr(d_tp), 2, hh, W, L.dptr(scores), L.dptr(ws), nb, 0, 0, None, st)
    assert fwd(off) == -1 and "4-byte aligned" in msg()
    assert fwd(None) == -1 and "null pointer" in msg()
    assert fwd(L.dptr(pf.rgbx), 1) == -1 and "H, W > 1" in msg()
    obj = lambda rgbx: lib.ivosw_assess_forward_objects_u8(L.dptr(packed), L.BF16, rgbx, 2, L.dptr(d_tp), H * W, 0, 1, H, W, L.dptr(scores),
                                                           L.dptr(ws), nb, 0, st)
    assert obj(off) == -1 and "4-byte aligned" in msg()
    assert obj(None) == -1 and "null pointer" in msg()
    torch.cuda.synchronize(dev)
    assert bool((sentinel == 7.0).all()) and bool((scores == 7.0).all()) and bool((out == 0xCD).all())        # nothing was launched
    assert obj(L.dptr(pf.rgbx)) == 0 and fwd(L.dptr(pf.rgbx)) == 0             # and the same calls with good arguments run
    torch.cuda.synchronize(dev)
    assert torch.isfinite(scores).all() and not bool((scores == 7.0).any())


# ---------------------------------------------------------------------------------------------- entry points
SMALL = ["setting=wild", "method=ours", "synth.n_sequences=1", "synth.n_frames=8", "synth.height=48", "synth.width=80",
         "eval_max_nb_interactions=2"]


def test_real_stack_gives_the_same_run_in_both_frame_modes(tmp_path, monkeypatch, capsys):
    """frames=uint8 on the real-stack branch (cv2's bytes, flipped and packed) against frames=float32 (the same bytes / 255): the same
    recommendations, predicted qualities and curve, line for line; the 8-bit run uploads no float video."""
    from ivos_w_amd import entry
    from tests.test_entry_points import _install_real_stack_doubles
    dev = torch.device("cuda:0")
    runs = {}
    for mode in ("float32", "uint8"):
        common = ["synthetic=0", f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/{mode}", f"frames={mode}"] + SMALL
        cfg = entry.parse_cli(["with"] + common)
        if mode == "float32":
            _install_real_stack_doubles(monkeypatch, tmp_path, cfg, dev)
            root = cfg.data.root_dir_davis
        cfg.data.root_dir_davis = root
        utils_agent.clear_frame_cache()
        up0 = utils_agent.frame_cache.uploads
        out = entry.run_eval(cfg, "MANet")
        text = capsys.readouterr().out
        assert out["backend"] == "real" and out["frames"] == mode and f"frames: {mode}" in text
        assert utils_agent.frame_cache.uploads - up0 == (1 if mode == "float32" else 0)
        runs[mode] = ([ln for ln in text.splitlines() if ln.startswith("avg_")], out["curve"], out["auc"])
    strip = lambda lines: [ln.split("rec_time:")[0] + ln.split("next_frame:")[1] for ln in lines]            # (the wall time differs)
    assert len(runs["uint8"][0]) == 2 and strip(runs["uint8"][0]) == strip(runs["float32"][0])
    assert runs["uint8"][1:] == runs["float32"][1:]
    utils_agent.clear_frame_cache()


def test_synthetic_session_runs_on_quantised_frames_and_says_so(tmp_path, capsys):
    from ivos_w_amd import entry
    cfg = entry.parse_cli(["with", "synthetic=1", "frames=uint8", f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/results"] + SMALL)
    dv = entry.SyntheticDavis(cfg, torch.device("cuda:0"))
    pf = dv.load_frames("synth-00")
    cfg32 = entry.parse_cli(["with", "synthetic=1"] + SMALL)
    f32 = entry.SyntheticDavis(cfg32, torch.device("cuda:0")).load_frames("synth-00")
    assert isinstance(pf, PackedFrames) and (pf.n, pf.H, pf.W) == (8, 48, 80)
    assert torch.equal(pf.rgbx[..., :3].cpu(), (f32 * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1))        # round(f * 255)
    utils_agent.clear_frame_cache()
    up0 = utils_agent.frame_cache.uploads
    out = entry.run_eval(cfg, "MANet")
    text = capsys.readouterr().out
    assert out["backend"] == "synthetic" and out["frames"] == "uint8"
    assert "frames=uint8" in text and "quantised" in text and "frames: uint8" in text
    assert utils_agent.frame_cache.uploads == up0 and len(out["curve"]["J_AND_F"]) == 2
