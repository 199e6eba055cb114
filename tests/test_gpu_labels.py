"""Label-map masks on the device (masks=labels): every *_lab entry and every host path that takes a LabelMasks against the EXISTING float
entries fed ``to_planes`` of the same map.  Everything is BIT FOR BIT: the label path is defined as the float path on the one-hot planes.
The shapes are the smallest that reach every branch: the 16-byte scan (40 x 64, aligned), the byte scan through the plane size (37 x 53,
H * W % 16 = 9) and through alignment (40 x 64, map base + 1 byte, odd frame stride), a float video mixed in, fp32 and RGBX8 frames."""
import ctypes
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models.assessment import AssessNet, LabelMasks, ScoreCache, pack_frames
from ivos_w_amd.utils import utils_agent

pytestmark = pytest.mark.gpu

DT = {"fp32": (L.F32, torch.float32), "bf16": (L.BF16, torch.bfloat16)}


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


def _net(dev, sd, prec, chunk=0):
    net = AssessNet(precision=prec, chunk=chunk)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def nets(dev, sd):
    return {prec: _net(dev, sd, prec) for prec in ("fp32", "bf16", "bf16x3")}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Vid:
    """One video of a call.  masks: a LabelMasks (a label video) or all_P [n,O+1,H,W] (a float video).  twin(): the float video on the
    one-hot planes of the map - what the label video is defined to equal."""

    def __init__(self, frames, masks, O):
        self.frames, self.masks, self.O = frames, masks, O
        self.u8 = not isinstance(frames, torch.Tensor)
        self.lab = isinstance(masks, LabelMasks)
        self.n, self.H, self.W = (frames.n, frames.H, frames.W) if self.u8 else (frames.shape[0], frames.shape[2], frames.shape[3])
        self.units, self.plane = self.n * self.O, self.H * self.W
        self._twin = None

    def triple(self):
        return (self.frames, self.masks, self.O)

    def twin(self):
        if not self.lab:
            return self
        if self._twin is None:
            self._twin = Vid(self.frames, self.masks.to_planes(self.O), self.O)
        else:
            self._twin.masks.copy_(self.masks.to_planes(self.O))               # in place: the float caches watch this storage
        return self._twin

    def desc(self):
        f = self.frames.rgbx if self.u8 else self.frames
        kind = L.FRAMES_RGBX8 if self.u8 else L.FRAMES_F32
        if self.lab:
            return L.Video(f.data_ptr(), None, 0, 0, kind, self.n, self.O, self.H, self.W)
        P = self.masks
        return L.Video(f.data_ptr(), P[:, 1:].data_ptr(), P.stride(0), P.stride(1), kind, self.n, self.O, self.H, self.W)

    def labels(self):
        if not self.lab:
            return L.Labels(None, 0)
        return L.Labels(self.masks.map.data_ptr(), self.masks.map.stride(0))


def _frames(dev, g, n, H, W, u8):
    if u8:
        return pack_frames(torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8), dev)
    return torch.rand(n, 3, H, W, generator=g).to(dev)


def _four(dev):
    """The table of four videos (21 units).  a: 40 x 64, aligned map, fp32 frames, 3 frames x 3 objects - the vector path; b: 37 x 53,
    RGBX8, 2 frames x 1 object - the byte path (H * W % 16 = 9); c: 40 x 64 with the map base 1 byte off and a frame stride of 2561,
    RGBX8, 2 frames x 3 objects - the byte path through alignment; d: a float video, 24 x 36, fp32 frames, 2 frames x 2 objects."""
    g = torch.Generator().manual_seed(99)
    H, W = 40, 64
    m = torch.zeros(3, H, W, dtype=torch.uint8)
    # frame 0: object 1 absent (empty box: the whole frame); object 2 = one pixel in each of the four corners; object 3 smaller than
    # 128 px in both extents (the minimum-extent rule)
    m[0, 0, 0] = m[0, 0, W - 1] = m[0, H - 1, 0] = m[0, H - 1, W - 1] = 2
    m[0, 17:22, 30:37] = 3
    # frame 1: object 1 = the top-left pixel alone, object 2 = the bottom-right pixel alone, object 3 touches all four borders
    m[1, 20, :] = 3
    m[1, :, 41] = 3
    m[1, 0, 0], m[1, H - 1, W - 1] = 1, 2
    # frame 2: object 1 = the top-right pixel, object 2 = the bottom-left pixel, object 3 a random blob; and the labels no unit may see
    m[2] = torch.where(torch.rand(H, W, generator=g) < 0.3, torch.tensor(3, dtype=torch.uint8), torch.tensor(0, dtype=torch.uint8))
    m[2, 0, W - 1], m[2, H - 1, 0] = 1, 2
    m[2, 5:9, 5:60] = 4                                                        # n_obj + 1
    m[2, 30:33, 2:50] = 255
    m[0, 3, 3:6] = 255
    a = Vid(_frames(dev, g, 3, H, W, False), LabelMasks(m.to(dev)), 3)
    assert a.masks.map.data_ptr() % 16 == 0 and a.plane % 16 == 0
    mb = torch.randint(0, 3, (2, 37, 53), generator=g, dtype=torch.uint8)      # labels 0, 1 and 2 = n_obj + 1
    mb[1] = 0
    mb[1, 36, 52] = 1                                                          # the last byte of the plane, in the tail behind the last vector
    mb[1, 10, 10] = 255
    b = Vid(_frames(dev, g, 2, 37, 53, True), LabelMasks(mb.to(dev)), 1)
    assert b.plane % 16 == 9
    mc = torch.randint(0, 5, (2, H, W), generator=g, dtype=torch.uint8)        # 0 .. 4: 4 = n_obj + 1
    mc[0, :, :20] = 1
    buf = torch.zeros(1 + 2 * 2561, dtype=torch.uint8, device=dev)
    view = buf[1:].as_strided((2, H, W), (2561, W, 1))
    view.copy_(mc.to(dev))
    c = Vid(_frames(dev, g, 2, H, W, True), LabelMasks(view), 3)
    assert c.masks.map.data_ptr() % 2 == 1 and c.masks.map.stride(0) == 2561
    P = torch.rand(2, 3, 24, 36, generator=g) * 0.45
    P[0, 1, 3:20, 5:30] = 0.8
    P[1, 2, 10:12, 20:22] = 0.9
    d = Vid(_frames(dev, g, 2, 24, 36, False), P.to(dev), 2)
    return [a, b, c, d]


def _table(vids):
    return (L.Video * len(vids))(*[v.desc() for v in vids])


def _labels(vids):
    return (L.Labels * len(vids))(*[v.labels() for v in vids])


def _firsts(vids):
    return np.concatenate([[0], np.cumsum([v.units for v in vids])]).astype(int)


# ---------------------------------------------------------------------------------------------- the front end alone
def test_front_end_equals_the_float_entries_on_the_planes(dev):
    lib, st, vids = L.lib(), L.stream_ptr(dev), _four(dev)
    twins = [v.twin() for v in vids]
    units = sum(v.units for v in vids)
    assert units == 21 and [v.O for v in vids] == [3, 1, 3, 2]
    arr, lab, tarr = _table(vids), _labels(vids), _table(twins)
    scratch = torch.empty(units, 4, dtype=torch.int32, device=dev)
    want = torch.empty(units, 4, device=dev)
    L.check(lib.ivosw_mask_bbox_videos(tarr, 4, L.dptr(want), L.dptr(scratch), st), "mask_bbox_videos")
    boxes = scratch.clone()                                                    # the integer boxes (ymin, ymax, xmin, xmax) before the margins
    scratch.fill_(-5)
    got = torch.full((units + 1, 4), float("nan"), device=dev)
    L.check(lib.ivosw_mask_bbox_videos_lab(arr, lab, 4, L.dptr(got), L.dptr(scratch), st), "mask_bbox_videos_lab")
    assert _same(got[:units], want) and bool(torch.isnan(got[units]).all())
    assert torch.equal(scratch, boxes)
    # the cases the maps were built for (a, frame-major inside an object: unit = obj * 3 + frame)
    bx = boxes.cpu().tolist()
    assert bx[0][1] == -1                                                      # object 1 absent from frame 0: the empty box
    assert bx[3] == [0, 39, 0, 63] and bx[7] == [0, 39, 0, 63]                 # the four corners; the object touching all four borders
    assert bx[1] == [0, 0, 0, 0] and bx[4] == [39, 39, 63, 63] and bx[2] == [0, 0, 63, 63] and bx[5] == [39, 39, 0, 0]       # one pixel
    assert bx[6] == [17, 21, 30, 36]                                           # smaller than 128 px
    assert bx[10] == [36, 36, 52, 52]                                          # b, frame 1: the last byte of a 1961-byte plane
    assert len({tuple(r) for r in bx}) >= 10                                   # the boxes differ: the comparison above means something
    # labels == NULL is the plain entry, on the float table
    got2 = torch.empty(units, 4, device=dev)
    L.check(lib.ivosw_mask_bbox_videos_lab(tarr, None, 4, L.dptr(got2), L.dptr(scratch), st), "mask_bbox_videos_lab")
    assert _same(got2, want)
    order = list(range(units))
    random.Random(5).shuffle(order)
    order[7] = units + 3                                                      # one id outside the table: a zero box, a zero tile
    ids = torch.tensor(order, dtype=torch.int32, device=dev)
    n = len(order)
    wu, gu = torch.empty(n, 4, device=dev), torch.full((n + 1, 4), float("nan"), device=dev)
    L.check(lib.ivosw_mask_bbox_units(tarr, 4, L.dptr(ids), n, L.dptr(wu), L.dptr(scratch.new_empty(n, 4)), st), "mask_bbox_units")
    L.check(lib.ivosw_mask_bbox_units_lab(arr, lab, 4, L.dptr(ids), n, L.dptr(gu), L.dptr(scratch.new_empty(n, 4)), st), "mask_bbox_units_lab")
    assert _same(gu[:n], wu) and bool((gu[7] == 0).all()) and bool(torch.isnan(gu[n]).all())
    inside = [i for i in range(n) if i != 7]
    assert _same(gu[inside], want[[order[i] for i in inside]])
    for name, (dt, tdt) in DT.items():
        wr = torch.empty(units, 256, 256, 4, dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_videos(tarr, 4, L.dptr(want), dt, L.dptr(wr), st), "roi_sample_videos")
        gr = torch.full((units + 1, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_videos_lab(arr, lab, 4, L.dptr(want), dt, L.dptr(gr), st), "roi_sample_videos_lab")
        assert _same(gr[:units], wr), name
        assert bool(torch.isnan(gr[units].float()).all())                      # nothing written behind the table
        p = wr[..., 3].float()
        assert float(p.min()) == 0.0 and float(p.max()) > 0.99 and bool(((p > 0.01) & (p < 0.99)).any())   # the mask channel: interpolated one-hot
        gr2 = torch.empty(units, 256, 256, 4, dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_videos_lab(tarr, None, 4, L.dptr(want), dt, L.dptr(gr2), st), "roi_sample_videos_lab")
        assert _same(gr2, wr), name
        wl = torch.empty(n, 256, 256, 4, dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_units(tarr, 4, L.dptr(ids), n, L.dptr(wu), dt, L.dptr(wl), st), "roi_sample_units")
        gl = torch.full((n + 1, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
        L.check(lib.ivosw_roi_sample_units_lab(arr, lab, 4, L.dptr(ids), n, L.dptr(gu), dt, L.dptr(gl), st), "roi_sample_units_lab")
        assert _same(gl[:n], wl) and bool((gl[7].float() == 0).all()) and bool(torch.isnan(gl[n].float()).all()), name
        assert _same(gl[inside], wr[[order[i] for i in inside]]), name


# ---------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("prec,chunk", [("fp32", 0), ("bf16", 0), ("bf16x3", 0), ("bf16", 4)])
def test_forward_videos_with_label_masks(dev, sd, nets, prec, chunk):
    """b, c, d: 12 units.  chunk = 4: the boundaries 4 | 8 fall inside c, a label video."""
    net = nets[prec] if chunk == 0 else _net(dev, sd, prec, chunk)
    vids = _four(dev)[1:]
    assert sum(v.units for v in vids) == 12
    want = net.forward_videos([v.twin().triple() for v in vids])
    got = net.forward_videos([v.triple() for v in vids])
    assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, want))
    assert float(torch.cat([w.reshape(-1) for w in want]).std()) > 0
    one = net.forward_objects(*vids[1].triple())                               # a LabelMasks in forward_objects: the same scores
    assert _same(one, want[1])
    if prec == "bf16" and chunk == 0:                                          # a plain uint8 tensor does NOT select the path: cast to float
        raw = vids[1].masks.map.contiguous()[:, None].expand(-1, 4, -1, -1)
        cast = net.forward_objects(vids[1].frames, raw, 3)
        assert _same(cast, net.forward_objects(vids[1].frames, raw.float(), 3))


# ---------------------------------------------------------------------------------------------- the delta pass
class Delta:
    """The caches of a table and of its float twin; run() calls the _lab entry on the one and the plain entry on the other."""

    def __init__(self, dev, vids):
        self.dev, self.vids, self.units = dev, vids, sum(v.units for v in vids)
        g = torch.Generator().manual_seed(7)
        self.cache, self.tcache = [], []
        for v in vids:
            junk = torch.randint(-2 ** 31, 2 ** 31 - 1, (v.units * v.plane,), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
            self.tcache.append(junk.view(torch.float32))
            if v.lab:                                                          # undefined content: every call starts cold
                self.cache.append(torch.randint(6, 250, (v.n * v.plane,), generator=g, dtype=torch.uint8).to(dev))
            else:
                self.cache.append(junk.clone().view(torch.float32))

    def _call(self, fn, args, caches, cold):
        meta = torch.full((2 * self.units + 3,), -77, dtype=torch.int32, device=self.dev)       # flags | guard | ids | guard | n | guard
        flags, ids, n = meta[:self.units], meta[self.units + 1:2 * self.units + 1], meta[2 * self.units + 2:2 * self.units + 3]
        ptrs = (ctypes.c_void_p * len(caches))(*[c.data_ptr() for c in caches])
        L.check(fn(*args, ptrs, L.int_array(cold), L.dptr(flags), L.dptr(ids), L.dptr(n), L.stream_ptr(self.dev)), "mask_delta")
        h = meta.cpu().numpy()
        assert h[self.units] == -77 and h[2 * self.units + 1] == -77           # nothing written beside the three outputs
        nd = int(h[2 * self.units + 2])
        return [int(u) for u in h[self.units + 1:self.units + 1 + nd]], h[:self.units].copy()

    def run(self, cold):
        lib, vids = L.lib(), self.vids
        twins = [v.twin() for v in vids]
        got, gflags = self._call(lib.ivosw_mask_delta_videos_lab, (_table(vids), _labels(vids), len(vids)), self.cache, cold)
        want, wflags = self._call(lib.ivosw_mask_delta_videos, (_table(twins), len(vids)), self.tcache, cold)
        assert got == want and got == sorted(got)                              # as a set and in order: what the float pass reports
        np.testing.assert_array_equal(gflags, wflags)
        for v, c in zip(vids, self.cache):                                     # the cache then equals the map
            if v.lab:
                assert torch.equal(c.view(v.n, v.H, v.W), v.masks.map)
        return got


def test_delta_cold_unchanged_and_single_pixels(dev):
    vids = _four(dev)
    first, units = _firsts(vids), 21
    D = Delta(dev, vids)
    none = [0, 0, 0, 0]
    assert D.run([1, 1, 1, 1]) == list(range(units))                           # cold: every unit, ascending; the map is copied
    before = [c.clone() for c in D.cache]
    assert D.run(none) == []                                                   # unchanged: nothing dirty ...
    assert all(torch.equal(a, b) for a, b in zip(before, D.cache))             # ... and the cache bytes as they were
    a, b, c = vids[0].masks.map, vids[1].masks.map, vids[2].masks.map

    def unit(vi, fr, label):
        return int(first[vi]) + (label - 1) * vids[vi].n + fr
    # one pixel a -> b dirties exactly (frame, a - 1) and (frame, b - 1); (video, frame, y, x, new label)
    cases = [(0, 1, 5, 5, 2),                                # a = 0: background -> object 2
             (0, 1, 5, 5, 0),                                # b = 0: object 2 -> background
             (0, 1, 5, 5, 3), (0, 1, 5, 5, 1),               # object -> object: two units
             (0, 2, 12, 12, 200),                            # b > n_obj: only the unit the pixel left (whatever it held)
             (0, 2, 12, 12, 4),                              # both outside 1 .. n_obj: nothing is dirty, the byte is still stored
             (0, 0, 0, 0, 1),                                # the first byte of a plane (a = 2)
             (0, 2, 39, 63, 2),                              # the last byte of the last plane of the map
             (1, 0, 36, 50, 1), (1, 0, 36, 50, 0),           # the byte path: in the tail behind the last full 16-byte vector of a 1961-byte plane
             (1, 1, 36, 52, 0),                              # ... and the plane's last byte
             (2, 1, 0, 0, 3), (2, 1, 39, 63, 2), (2, 0, 7, 3, 0)]      # the misaligned map: first and last byte of a frame
    for vi, fr, y, x, new in cases:
        m = vids[vi].masks.map
        old = int(m[fr, y, x])
        if old == new:
            new = new % 3 + 1
        m[fr, y, x] = new
        want = sorted(unit(vi, fr, l) for l in {old, new} if 1 <= l <= vids[vi].O)
        assert D.run(none) == want, (vi, fr, y, x, old, new)
        assert D.run(none) == []
    # several at once, across videos and kinds, plus a label above 64 (no unit here owns it: nothing flagged, nothing out of bounds)
    a[0, 10, 10], a[2, 0, 0], b[1, 0, 0], c[0, 39, 0] = 1, 70, 1, 2
    vids[3].masks[1, 2, 0, 0] += 0.25
    got = D.run(none)
    assert unit(0, 0, 1) in got and unit(1, 1, 1) in got and unit(2, 0, 2) in got and int(first[3]) + 1 * 2 + 1 in got
    assert D.run(none) == []
    # cold for one label video only
    a[1, 3, 3] = 1
    assert D.run([0, 1, 0, 0]) == [unit(0, 1, 1)] + list(range(int(first[1]), int(first[2])))
    assert D.run(none) == []


def test_delta_labels_above_64_take_the_store_path(dev):
    """n_obj = 100 on a 20 x 16 map (the vector path) and a 5 x 7 one (bytes): labels 65 .. 100 are flagged by the plain store."""
    g = torch.Generator().manual_seed(3)
    vids = [Vid(_frames(dev, g, 2, 20, 16, False), LabelMasks(torch.randint(0, 101, (2, 20, 16), generator=g, dtype=torch.uint8).to(dev)), 100),
            Vid(_frames(dev, g, 1, 5, 7, False), LabelMasks(torch.randint(0, 101, (1, 5, 7), generator=g, dtype=torch.uint8).to(dev)), 100)]
    D = Delta(dev, vids)
    assert D.run([1, 1]) == list(range(300))
    assert D.run([0, 0]) == []
    for vi, fr, y, x, new in ((0, 1, 19, 15, 100), (0, 0, 0, 0, 65), (1, 0, 4, 6, 99), (0, 1, 7, 7, 64)):
        m = vids[vi].masks.map
        old = int(m[fr, y, x])
        new = new if new != old else new - 1
        m[fr, y, x] = new
        want = sorted(200 * vi + (l - 1) * vids[vi].n + fr for l in {old, new} if l >= 1)
        assert D.run([0, 0]) == want, (vi, fr, y, x, old, new)


# ---------------------------------------------------------------------------------------------- sequences
def test_forward_incremental_with_label_masks_through_in_place_edits(dev, nets):
    net, vids = nets["bf16"], _four(dev)[1:]                                   # b, c (label videos), d (float): 2 + 6 + 4 units
    caches, tcaches = [ScoreCache() for _ in vids], [ScoreCache() for _ in vids]

    def call(expect):
        got = net.forward_videos_incremental([v.triple() for v in vids], caches)
        want = net.forward_videos([v.triple() for v in vids])
        assert all(_same(x, y) for x, y in zip(got, want))
        twin = net.forward_videos_incremental([v.twin().triple() for v in vids], tcaches)      # ... and the float path on the planes
        assert all(_same(x, y) for x, y in zip(got, twin))
        assert [c.rescored for c in caches] == list(expect) == [c.rescored for c in tcaches]
        return want
    w0 = call([2, 6, 4])                                                       # cold
    assert caches[0].planes.dtype == torch.uint8 and caches[0].planes.numel() == 2 * 37 * 53
    assert caches[2].planes.dtype == torch.float32
    assert caches[1].nbytes == ScoreCache.nbytes_for(2, 3, 40, 64, "labels")
    call([0, 0, 0])
    b, c = vids[0].masks.map, vids[1].masks.map
    c[1, 10:20, 10:30] = 2                                                     # frame 1 of c: object 2 grows over whatever was there
    w1 = call([0, 3, 0])
    assert not _same(w1[1], w0[1]) and _same(w1[0], w0[0])
    b[0, 0:5, 0:5] = 1
    c[0, 0, 0] = 0                                                             # was object 1
    vids[2].masks[0, 1].mul_(0.5)
    call([1, 1, 1])
    y, x = (int(t) for t in (c[0] == 4).nonzero()[0])
    c[0, y, x] = 0                                                             # between two labels no object owns: nothing to score
    call([0, 0, 0])
    # the other mask kind on the same frames and caches: cold
    swapped = [ScoreCache() for _ in vids]
    net.forward_videos_incremental([v.triple() for v in vids], swapped)
    net.forward_videos_incremental([v.twin().triple() for v in vids], swapped)
    assert [s.rescored for s in swapped] == [2, 6, 0] and swapped[0].planes.dtype == torch.float32


def _agent(dev, **options):
    from ivos_w_amd.models.agent import Agent
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4, **options))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    return agent


@pytest.mark.parametrize("rescore", ["all", "changed"])
def test_recommend_candidates_under_labels_equals_float_on_the_planes(dev, nets, rescore):
    net = nets["bf16"]
    g = torch.Generator().manual_seed(31)
    vids = []
    for n, O, H, W, u8 in ((6, 2, 24, 32, False), (4, 1, 31, 27, True), (5, 3, 18, 40, False)):
        m = torch.randint(0, O + 2, (n, H // 4 + 1, W // 4 + 1), generator=g, dtype=torch.uint8)         # blocky labels, 0 .. n_obj + 1
        m = m.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
        vids.append(Vid(_frames(dev, g, n, H, W, u8), LabelMasks(m if len(vids) == 1 else m.to(dev)), O))        # one map on the host: uploaded
    cy = AD(setting="wild", method="ours", rescore=rescore)
    agents = (_agent(dev, candidates=3, skip_annotated=True), _agent(dev, candidates=3, skip_annotated=True))
    utils_agent.clear_score_cache()
    utils_agent.clear_frame_cache()

    def requests(labels):
        out = []
        for v in vids:
            P = v.masks if labels else Vid(v.frames, v.masks.to(dev), v.O).twin().masks
            out.append(dict(n_frame=v.n, n_objects=v.O, all_F=v.frames, all_P=P, new_masks_quality=np.zeros(v.n), prev_frames=[1],
                            annotated_frames_list=[1, 1, 0], mask_quality=np.zeros(v.n), first_frame=1, max_nb_interactions=8))
        return out
    for it in range(2):
        if it == 1:
            vids[0].masks.map[2, 4:12, 4:12] = 1
            vids[2].masks.map[0] = 0
        for pick in (slice(0, 3), slice(1, 2)):                                # three sessions in one pass; one session (its own chain)
            res = []
            for labels, agent in zip((False, True), agents):
                random.seed(3)
                np.random.seed(3)
                reqs = requests(labels)[pick]
                res.append(([np.asarray(r).tolist() for r in utils_agent.recommend_candidates(cy, net, agent, dev, reqs)],
                            [r["mask_quality"].copy() for r in reqs]))
            (want, wq), (got, gq) = res
            assert got == want and all(len(c) == 3 for c in got)
            for x, y in zip(gq, wq):
                np.testing.assert_array_equal(x, y)                            # mask_quality, bit for bit
                assert np.ptp(x) > 0
    # assess_all_objects / assess_videos_device take a LabelMasks in all_P's place
    v = vids[0]
    np.testing.assert_array_equal(utils_agent.assess_all_objects(net, v.frames, v.masks, v.O, dev, rescore=rescore),
                                  utils_agent.assess_all_objects(net, v.frames, v.twin().masks, v.O, dev))
    if rescore == "changed":                                                   # the LRU counts the label sessions' real bytes
        lab_bytes = sum(ScoreCache.nbytes_for(v.n, v.O, v.H, v.W, "labels") for v in vids)
        f32_bytes = sum(ScoreCache.nbytes_for(v.n, v.O, v.H, v.W) for v in vids)
        assert utils_agent.score_cache.nbytes() == lab_bytes + f32_bytes
    utils_agent.clear_score_cache()
    utils_agent.clear_frame_cache()


# ---------------------------------------------------------------------------------------------- refusals
def test_lab_refusals_on_device_pointers(dev, nets):
    lib, st, vids = L.lib(), L.stream_ptr(dev), _four(dev)
    msg = lambda: lib.ivosw_last_error().decode()
    out = torch.full((32, 4), 7.0, device=dev)
    scratch = torch.zeros(32, 4, dtype=torch.int32, device=dev)

    def bbox(arr, lab):
        return lib.ivosw_mask_bbox_videos_lab(arr, lab, 4, L.dptr(out), L.dptr(scratch), st)
    arr = _table(vids)
    arr[0].n_obj = 256
    assert bbox(arr, _labels(vids)) == -1 and "video 0" in msg() and "255" in msg()
    lab = _labels(vids)
    lab[2].stride_frame = 40 * 64 - 1                                          # overlapping frames
    assert bbox(_table(vids), lab) == -1 and "video 2" in msg() and "overlap" in msg()
    lab[2].stride_frame = -2561
    assert bbox(_table(vids), lab) == -1 and "video 2" in msg() and "negative" in msg()
    lab = _labels(vids)
    lab[1].map = None                                                          # b becomes a float video, and its masks are NULL
    assert bbox(_table(vids), lab) == -1 and "video 1" in msg() and "null pointer" in msg()
    assert bbox(_table(vids), None) == -1 and "video 0" in msg() and "null pointer" in msg()
    net = nets["bf16"]
    packed = net._ensure_packed()
    nb = lib.ivosw_assess_ws_bytes(L.BF16, 21, 2, 2, 0)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    arr = _table(vids)
    arr[2].n_obj = 300
    assert lib.ivosw_assess_forward_videos_lab(L.dptr(packed), L.BF16, arr, _labels(vids), 4, L.dptr(out), L.dptr(ws), nb, 0, 0, None, st) == -1
    assert "video 2" in msg() and "255" in msg()
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all()) and bool((scratch == 0).all())             # nothing was launched
    # labels == NULL through the forward: the plain entry, bit for bit
    twins = [v.twin() for v in vids]
    want, got = torch.empty(21, device=dev), torch.empty(21, device=dev)
    L.check(lib.ivosw_assess_forward_videos(L.dptr(packed), L.BF16, _table(twins), 4, L.dptr(want), L.dptr(ws), nb, 0, 0, None, st), "fwd")
    L.check(lib.ivosw_assess_forward_videos_lab(L.dptr(packed), L.BF16, _table(twins), None, 4, L.dptr(got), L.dptr(ws), nb, 0, 0, None, st), "fwd")
    assert _same(got, want)
    L.check(lib.ivosw_assess_forward_videos_lab(L.dptr(packed), L.BF16, _table(vids), _labels(vids), 4, L.dptr(got), L.dptr(ws), nb, 0, 0, None,
                                                st), "fwd")
    assert _same(got, want)
