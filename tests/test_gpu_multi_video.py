"""Several videos in one assessment pass: the descriptor-driven front end (ivosw_mask_bbox_videos / ivosw_roi_sample_videos), the whole
forward (ivosw_assess_forward_videos, AssessNet.forward_videos) through chunk boundaries and the two-stream split, and
utils_agent.recommend_frames return BIT FOR BIT what the single-video entries return per video.  No tolerance is introduced: the
single-video entries are pinned against the reference goldens by the existing tests, and the multi-video path is defined as equal to
them."""
import copy
import ctypes
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models.assessment import AssessNet, PackedFrames, pack_frames
from ivos_w_amd.utils import utils_agent

pytestmark = pytest.mark.gpu


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()}


@pytest.fixture(scope="module")
def nets(dev, sd):
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


def _rect(H, W, y0, y1, x0, x1, g):
    """A soft mask: > 0.5 exactly inside rows y0..y1, columns x0..x1 (inclusive), noise below 0.5 elsewhere."""
    m = torch.rand(H, W, generator=g) * 0.45
    m[y0:y1 + 1, x0:x1 + 1] = 0.55 + 0.45 * torch.rand(y1 - y0 + 1, x1 - x0 + 1, generator=g)
    return m


class Vid:
    """One video of a call: frames (fp32 [n,3,H,W] or PackedFrames), all_P (any layout forward_objects takes), n objects."""

    def __init__(self, frames, all_P, O):
        self.frames, self.all_P, self.O = frames, all_P, O
        self.u8 = isinstance(frames, PackedFrames)
        self.n, self.H, self.W = (frames.n, frames.H, frames.W) if self.u8 else (frames.shape[0], frames.shape[2], frames.shape[3])
        self.units = self.n * self.O

    def triple(self):
        return (self.frames, self.all_P, self.O)

    def desc(self):
        f = self.frames.rgbx if self.u8 else self.frames
        return L.Video(f.data_ptr(), self.all_P[:, 1:].data_ptr(), self.all_P.stride(0), self.all_P.stride(1),
                       L.FRAMES_RGBX8 if self.u8 else L.FRAMES_F32, self.n, self.O, self.H, self.W)

    def unit_masks(self):
        """[units,H,W] contiguous, unit u = obj * n + frame: what the single-video entries read."""
        return self.all_P[:, 1:1 + self.O].permute(1, 0, 2, 3).reshape(self.units, self.H, self.W).contiguous()

    def unit_frames(self):
        """The frames replicated per object, as the single-video entries without the frame indirection want them."""
        if self.u8:
            return PackedFrames(self.frames.rgbx.repeat(self.O, 1, 1, 1).contiguous())
        return self.frames.repeat(self.O, 1, 1, 1).contiguous()


def _random_video(dev, g, n, O, H, W, u8=False, object_major=False):
    if u8:
        frames = pack_frames(torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8), dev)
    else:
        frames = torch.rand(n, 3, H, W, generator=g).to(dev)
    if object_major:                                                           # the ProbStore view: storage [C,n,H,W], seen as [n,C,H,W]
        all_P = torch.rand(O + 1, n, H, W, generator=g).to(dev).permute(1, 0, 2, 3)
    else:
        all_P = torch.rand(n, O + 1, H, W, generator=g).to(dev)
    return Vid(frames, all_P, O)


@pytest.fixture(scope="module")
def mixed(dev):
    """The videos of the front-end test.  a: 40 x 56 fp32 (plane % 4 == 0: the 16-byte scan), 3 frames x 2 objects in an
    [n,O+1,H,W] all_P; b: 37 x 51 fp32 (odd plane: the scalar scan), 2 frames x 1 object, object-major strides; c: 33 x 47 RGBX8, 1 frame x
    3 objects; d: 2 x 2; e: a 6 x 300 strip, 1 frame x 2 objects - frames below ~200 pixels clip every grown box to the same
    (-5 .. H + 5, -5 .. W + 5), so this one carries the case of two objects of a frame with different (y,x,h,w): a 241-pixel box (no grow
    in x) and an 11-pixel box.  Masks: a / frame 0 has a different box per object, a / frame 1 / object 0 is empty (the whole-frame box with this
    video's H, W), a / frame 2 / object 1 touches all four borders; b holds a 5 x 7 box (far below 128 pixels: the grow branch, which every
    box of frames this small takes) and a one-pixel box in the last row and column; c: empty, full and a corner box; d: one pixel."""
    g = torch.Generator().manual_seed(1234)
    a = _random_video(dev, g, 3, 2, 40, 56)
    P = torch.rand(3, 3, 40, 56, generator=g) * 0.45
    P[0, 1], P[0, 2] = _rect(40, 56, 3, 20, 5, 30, g), _rect(40, 56, 25, 38, 40, 55, g)
    P[1, 1], P[1, 2] = torch.zeros(40, 56), _rect(40, 56, 10, 11, 20, 21, g)
    P[2, 1], P[2, 2] = _rect(40, 56, 17, 23, 0, 9, g), _rect(40, 56, 0, 39, 0, 55, g)
    a.all_P = P.to(dev)
    b = _random_video(dev, g, 2, 1, 37, 51, object_major=True)
    Pb = torch.rand(2, 2, 37, 51, generator=g) * 0.45                          # [C,n,H,W]
    Pb[1, 0], Pb[1, 1] = _rect(37, 51, 12, 16, 30, 36, g), _rect(37, 51, 36, 36, 50, 50, g)
    b.all_P = Pb.to(dev).permute(1, 0, 2, 3)
    assert b.all_P.stride(0) == 37 * 51 and b.all_P.stride(1) == 2 * 37 * 51
    c = _random_video(dev, g, 1, 3, 33, 47, u8=True)
    Pc = torch.rand(1, 4, 33, 47, generator=g) * 0.45
    Pc[0, 1], Pc[0, 2], Pc[0, 3] = torch.zeros(33, 47), torch.ones(33, 47), _rect(33, 47, 0, 4, 0, 6, g)
    c.all_P = Pc.to(dev)
    d = _random_video(dev, g, 1, 1, 2, 2)
    d.all_P = torch.tensor([[[[0.1, 0.2], [0.3, 0.4]], [[0.0, 0.0], [0.0, 0.9]]]]).to(dev)
    e = _random_video(dev, g, 1, 2, 6, 300)
    Pe = torch.rand(1, 3, 6, 300, generator=g) * 0.45
    Pe[0, 1], Pe[0, 2] = _rect(6, 300, 1, 4, 10, 250, g), _rect(6, 300, 0, 5, 280, 290, g)
    e.all_P = Pe.to(dev)
    return [a, b, c, d, e]


def _table(vids):
    return (L.Video * len(vids))(*[v.desc() for v in vids])


# ---------------------------------------------------------------------------------------------- the front end alone
def _boxes_single(dev, v):
    lib = L.lib()
    m = v.unit_masks()
    out = torch.full((v.units, 4), float("nan"), device=dev)
    scratch = torch.empty(v.units, 4, dtype=torch.int32, device=dev)
    L.check(lib.ivosw_mask_bbox(L.dptr(m), v.units, v.H, v.W, L.dptr(out), L.dptr(scratch), L.stream_ptr(dev)), "mask_bbox")
    return out


def test_front_end_equals_the_single_video_kernels(dev, mixed):
    lib, st = L.lib(), L.stream_ptr(dev)
    arr = _table(mixed)
    units = int(lib.ivosw_assess_videos_units(arr, len(mixed)))
    assert units == 6 + 2 + 3 + 1 + 2
    got = torch.full((units + 1, 4), float("nan"), device=dev)                 # one guard row behind the last unit
    scratch = torch.empty(units, 4, dtype=torch.int32, device=dev)
    L.check(lib.ivosw_mask_bbox_videos(arr, len(mixed), L.dptr(got), L.dptr(scratch), st), "mask_bbox_videos")
    want = torch.cat([_boxes_single(dev, v) for v in mixed])
    assert bool(torch.isnan(got[units]).all())
    assert _same(got[:units], want)
    # the masks do what the docstring of `mixed` says: the empty mask of video a gives the whole-frame box of a 40 x 56 frame, that of
    # video c the box of a 33 x 47 frame; the two objects of e's frame have different boxes
    h = want.cpu()
    assert not torch.equal(h[12], h[13]) and not torch.equal(h[1], h[8]) and torch.isfinite(h).all()
    for dtype, tdt in ((L.F32, torch.float32), (L.BF16, torch.bfloat16)):
        roi = torch.full((units + 1, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_videos(arr, len(mixed), L.dptr(want), dtype, L.dptr(roi), st), "roi_sample_videos")
        off = 0
        for v in mixed:
            ref = torch.full((v.units, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
            f, m, bx = v.unit_frames(), v.unit_masks(), want[off:off + v.units].contiguous()
            if v.u8:
                L.check(lib.ivosw_roi_sample_u8(L.dptr(f.rgbx), L.dptr(m), L.dptr(bx), v.units, v.H, v.W, dtype, L.dptr(ref), st), "roi_sample_u8")
            else:
                L.check(lib.ivosw_roi_sample(L.dptr(f), L.dptr(m), L.dptr(bx), v.units, v.H, v.W, dtype, L.dptr(ref), st), "roi_sample")
            assert not bool(torch.isnan(ref.float()).any())
            assert _same(roi[off:off + v.units], ref), (dtype, off)
            off += v.units
        assert bool(torch.isnan(roi[units].float()).all())                     # nothing written behind the last unit


# ---------------------------------------------------------------------------------------------- the whole forward
@pytest.fixture(scope="module")
def per_video_scores(nets, mixed):
    """forward_objects per video and precision: computed once, shared by the tests below."""
    return {prec: [net.forward_objects(*v.triple()).clone() for v in mixed] for prec, net in nets.items()}


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_forward_videos_equals_forward_objects_per_video(dev, sd, nets, mixed, per_video_scores, prec):
    vids, want = mixed[:3], per_video_scores[prec][:3]
    got = nets[prec].forward_videos([v.triple() for v in vids])
    assert len(got) == 3 and [tuple(s.shape) for s in got] == [(2, 3), (1, 2), (3, 1)]
    assert all(_same(s, w) for s, w in zip(got, want))
    assert all(s.data_ptr() == got[0].data_ptr() + 4 * o for s, o in zip(got, (0, 6, 8)))          # views of ONE flat tensor, unit order
    assert float(torch.cat([w.reshape(-1) for w in want]).std()) > 0
    # chunk = 4 over 11 units: chunks [0,4) [4,8) [8,11) - the first ends inside video a, the second spans a and b, the third starts at c
    small = AssessNet(precision=prec, chunk=4)
    small.load_state_dict(sd, strict=True)
    small = small.to(dev).eval()
    got4 = small.forward_videos([v.triple() for v in vids])
    assert all(_same(s, w) for s, w in zip(got4, want))
    # a single-video list is forward_objects
    for v, w in zip(vids, want):
        (one,) = nets[prec].forward_videos([v.triple()])
        assert _same(one, w)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_roi_tap_through_the_c_entry(dev, nets, mixed, prec):
    lib, net, vids = L.lib(), nets[prec], mixed[:3]
    dt = {"fp32": L.F32, "bf16": L.BF16, "bf16x3": L.F32X3}[prec]
    arr, units = _table(vids), 11
    packed = net._ensure_packed()
    nb = lib.ivosw_assess_ws_bytes(dt, units, 40, 56, units)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    scores = torch.full((units,), float("nan"), device=dev)
    tap = torch.full((units, 256, 256, 4), float("nan"), dtype=torch.bfloat16 if prec == "bf16" else torch.float32, device=dev)
    L.check(lib.ivosw_assess_forward_videos(L.dptr(packed), dt, arr, 3, L.dptr(scores), L.dptr(ws), nb, units, 1, L.dptr(tap),
                                            L.stream_ptr(dev)), "assess_forward_videos")
    ref = [net.forward_tap(v.unit_frames(), v.unit_masks(), "roi") for v in vids]
    assert _same(tap, torch.cat([t for _, t in ref]))
    assert _same(scores, torch.cat([s for s, _ in ref]))


def test_two_stream_split_inside_a_video(dev, nets):
    """70 units in bf16 with the default chunk: the pass splits at unit 40, inside the second video (units 39 .. 56)."""
    net, lib = nets["bf16"], L.lib()
    g = torch.Generator().manual_seed(77)
    vids = [_random_video(dev, g, 13, 3, 24, 36), _random_video(dev, g, 9, 2, 20, 28, u8=True), _random_video(dev, g, 13, 1, 30, 22)]
    assert sum(v.units for v in vids) == 70 and lib.ivosw_assess_split(L.BF16, 70, 0) == 1
    got = net.forward_videos([v.triple() for v in vids])
    for s, v in zip(got, vids):
        assert _same(s, net.forward_objects(*v.triple()))


def test_order_and_grouping(dev, nets, mixed, per_video_scores):
    net, want = nets["bf16"], per_video_scores["bf16"]
    perm = [2, 0, 3, 1]
    got = net.forward_videos([mixed[i].triple() for i in perm])
    assert all(_same(s, want[i]) for s, i in zip(got, perm))
    # 33 one-unit videos: a group of 32 and a group of one
    g = torch.Generator().manual_seed(5)
    tiny = [_random_video(dev, g, 1, 1, 6 + k % 5, 9 + k % 3, u8=(k % 4 == 1)) for k in range(33)]
    got = net.forward_videos([v.triple() for v in tiny])
    assert len(got) == 33 and all(tuple(s.shape) == (1, 1) for s in got)
    ref = torch.cat([net.forward_objects(*v.triple()).reshape(-1) for v in tiny])
    assert _same(torch.cat([s.reshape(-1) for s in got]), ref) and float(ref.std()) > 0


# ---------------------------------------------------------------------------------------------- recommend_frames
@pytest.mark.parametrize("method", ["ours", "worst"])
def test_recommend_frames_equals_recommend_frame_per_request(dev, nets, monkeypatch, method):
    from ivos_w_amd.models.agent import Agent
    net = nets["bf16"]
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    twin = copy.deepcopy(agent)
    g = torch.Generator().manual_seed(99)
    vids = [_random_video(dev, g, 6, 2, 24, 36), _random_video(dev, g, 4, 1, 31, 27, u8=True), _random_video(dev, g, 9, 3, 18, 40)]
    vids[2].frames = vids[2].frames.cpu()                                      # a host-resident all_F: uploaded for the call

    def requests():
        return [dict(n_frame=v.n, n_objects=v.O, all_F=v.frames, all_P=v.all_P, new_masks_quality=np.zeros(v.n), prev_frames=[1],
                     annotated_frames_list=[1, 1, 0], mask_quality=np.zeros(v.n), first_frame=1, max_nb_interactions=8) for v in vids]
    cy = AD(setting="wild", method=method)
    utils_agent.clear_frame_cache()
    random.seed(3)
    np.random.seed(3)
    want_req = requests()
    want = [int(utils_agent.recommend_frame(cy, net, twin, dev, **r)) for r in want_req]
    rng_want = (random.random(), float(np.random.rand()))
    utils_agent.clear_frame_cache()
    up0, hit0 = utils_agent.frame_cache.uploads, utils_agent.frame_cache.hits
    random.seed(3)
    np.random.seed(3)
    got_req = requests()
    copies = []
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    got = [int(i) for i in utils_agent.recommend_frames(cy, net, agent, dev, got_req)]
    monkeypatch.undo()
    assert copies == ["cpu"], copies                                           # ONE device-to-host copy for the whole call
    assert (utils_agent.frame_cache.uploads, utils_agent.frame_cache.hits) == (up0, hit0)
    assert got == want and all(0 <= i < v.n for i, v in zip(got, vids))
    for a, b in zip(got_req, want_req):
        np.testing.assert_array_equal(a["mask_quality"], b["mask_quality"])
        assert np.ptp(a["mask_quality"]) > 0
    assert agent.steps_done == twin.steps_done == (3 if method == "ours" else 0)
    assert (random.random(), float(np.random.rand())) == rng_want              # the host RNG streams moved as under sequential calls
    utils_agent.clear_frame_cache()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_video_and_launch_nothing(dev, nets, mixed):
    lib, net, st = L.lib(), nets["bf16"], L.stream_ptr(dev)
    msg = lambda: lib.ivosw_last_error().decode()
    vids = mixed[:3]
    packed = net._ensure_packed()
    nb = lib.ivosw_assess_ws_bytes(L.BF16, 11, 40, 56, 0)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    scores = torch.full((16,), 7.0, device=dev)

    def fwd(arr, n=3, dtype=L.BF16, pk=packed, sc=scores, w=ws):
        return lib.ivosw_assess_forward_videos(L.dptr(pk) if pk is not None else None, dtype, arr, n, L.dptr(sc) if sc is not None else None,
                                               L.dptr(w) if w is not None else None, nb, 0, 0, None, st)

    def broken(i, **kw):
        arr = _table(vids)
        for k, val in kw.items():
            setattr(arr[i], k, val)
        return arr
    cases = [(broken(1, frames=None), "video 1", "null pointer"), (broken(2, masks=None), "video 2", "null pointer"),
             (broken(0, frames_kind=2), "video 0", "frames_kind"), (broken(0, frames_kind=-1), "video 0", "frames_kind"),
             (broken(1, n_frames=0), "video 1", "positive"), (broken(2, n_obj=0), "video 2", "positive"), (broken(2, n_obj=-3), "video 2", "positive"),
             (broken(0, H=1), "video 0", "H, W > 1"), (broken(1, W=1), "video 1", "H, W > 1"), (broken(1, W=0), "video 1", "H, W > 1"),
             (broken(2, H=65536, W=32768), "video 2", "INT_MAX"),
             (broken(0, mask_stride_frame=-1), "video 0", "negative"), (broken(1, mask_stride_obj=-8), "video 1", "negative"),
             (broken(0, mask_stride_frame=40 * 56 - 1), "video 0", "overlap"),
             (broken(2, frames=vids[2].frames.rgbx.data_ptr() + 2), "video 2", "4-byte aligned"),
             (broken(1, n_frames=1 << 15, n_obj=1 << 15, mask_stride_frame=37 * 51), "video 1", "too many")]
    for arr, who, what in cases:
        assert fwd(arr) == -1 and who in msg() and what in msg(), (who, what, msg())
        assert lib.ivosw_assess_videos_units(arr, 3) == -1 and who in msg()
        assert lib.ivosw_mask_bbox_videos(arr, 3, L.dptr(scores), L.dptr(scores), st) == -1 and who in msg()
        assert lib.ivosw_roi_sample_videos(arr, 3, L.dptr(scores), L.F32, L.dptr(scores), st) == -1 and who in msg()
    # the total: 2^30 units spread over two videos, refused at the video that crosses the line
    arr = broken(0, n_frames=1 << 15, n_obj=1 << 14)
    arr[1].n_frames, arr[1].n_obj, arr[1].mask_stride_frame = 1 << 15, 1 << 14, 37 * 51
    assert fwd(arr) == -1 and "video 1" in msg() and "too many" in msg()
    good = _table(vids)
    for n in (0, -1, 33):
        assert fwd(good, n=n) == -1 and "n_videos" in msg() and str(n) in msg()
        assert lib.ivosw_assess_videos_units(good, n) == -1
    assert fwd(None) == -1 and "null pointer" in msg()
    assert fwd(good, dtype=7) == -1 and "dtype" in msg()
    assert lib.ivosw_roi_sample_videos(good, 3, L.dptr(scores), 7, L.dptr(scores), st) == -1 and "dtype" in msg()
    assert fwd(good, pk=None) == -1 and "null pointer" in msg()
    assert fwd(good, sc=None) == -1 and "null pointer" in msg()
    assert fwd(good, w=None) == -1 and "null pointer" in msg()
    assert fwd(good, dtype=L.F32) == -1 and "another dtype" in msg()           # the arena was packed for bf16
    assert lib.ivosw_assess_forward_videos(L.dptr(packed), L.BF16, good, 3, L.dptr(scores), L.dptr(ws), nb, 0, 1, None, st) == -1 and "tap_out" in msg()
    assert lib.ivosw_assess_forward_videos(L.dptr(packed), L.BF16, good, 3, L.dptr(scores), L.dptr(ws), 16, 0, 0, None, st) == -2 and "workspace" in msg()
    torch.cuda.synchronize(dev)
    assert bool((scores == 7.0).all())                                         # nothing was launched: the sentinel stands
    assert lib.ivosw_assess_videos_units(good, 3) == 11
    assert fwd(good) == 0
    torch.cuda.synchronize(dev)
    assert bool((scores[:11] != 7.0).all()) and bool((scores[11:] == 7.0).all())
