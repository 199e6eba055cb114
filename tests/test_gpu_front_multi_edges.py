"""The table-driven front end (csrc/assess_front.hip: video tables, unit lists, label maps) at its kernel edges, through the C ABI.
Everything is integer or bit-exact work: the boxes against oracle/front_ref.py (bbox_ref, bbox_minmax_ref, label_planes - pinned on
the CPU by tests/test_oracle_front_multi.py, which also shows that the lone-pixel positions and byte values used here tell a wrong
carry, a dropped vector and a sloppy byte test from the right scan), the dirty lists against label_delta_ref / the edits made, the
tiles against the single-video sampler that tests/test_gpu_front_edges.py holds to float64.  Every output has a guard row behind it.

  loop / branch of assess_front.hip                          reached by
  bbox_scan_multi float4: 4-loads loop + tail, S = 64         test_float_box_workload_plane_at_every_seam (480 x 854, chunk 7168: seven
                                                             strides per chunk, sy = 1, sx = 170, a wrap every few steps)
  ... carried (y, x) at W > 1024 (sy = 0), W = 1024 (sx = 0)  test_float_box_carried_coordinates (70 x 1100 + 80 x 1024, chunk 2048)
  ... S = 1 (units > 2048), W = 2, 4-loads loop every lane    test_float_box_one_chunk_per_unit (4 x 1025, 4 x 1024, 4 x 1100, 2048 x 2, 8 x 8)
  ... planes of different sizes, early exit, scalar scan      test_float_box_mixed_table (480 x 854 ... 2 x 2, strided all_P, base + 4 bytes)
  bbox_scan_multi label: tail loop carries (chunk 7168)       test_label_box_workload_plane[32]
  ... 4 x 4096 loop carries (chunk 26624)                     test_label_box_workload_plane[128]
  ... S = 1, 4 x 4096 loop + tail, W > / = 1024               test_label_box_one_chunk_per_unit (16 x 1100, 16 x 1024, 37 x 53)
  ... has_byte next to label ^ 0x80, +- 1, 0, 255; n_obj 255  test_label_box_hard_byte_values
  ... float + label + RGBX8 label video in one table          test_label_box_mixed_table
  byte scan of a label map (base + 1 byte, odd plane)         every label test above, second layout
  UnitList (S from n_ids, ids -1 and units, repeats)          test_unit_lists_* on the tables above, n_ids 1, 33, > 2048
  delta_compact: base loop, running total (> 1024 flags)      test_delta_compaction_beyond_one_round (1023 ... 3001 units, 32 videos)
  mask_delta_lab: second slice, 4 x 4096 loop, labels > 64    test_label_delta_beyond_one_slice (480 x 854: 26 slices; 130 x 128; 131 x 127 bytes)
  ... ffirst lookup with a float video between label videos   test_delta_table_label_float_label
  roi_sample_multi at workload size, boxes inside the frame   test_sampler_at_workload_size (480 x 854 + 150 x 200, fp32 / RGBX8, labels, lists)
"""
import ctypes

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from oracle import front_ref as fr

pytestmark = pytest.mark.gpu

SENT = -77
DT = {"fp32": (L.F32, torch.float32), "bf16": (L.BF16, torch.bfloat16)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _shifted(t, by=1):
    """The same values in a buffer that starts `by` elements behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[by:by + t.numel()]
    v.copy_(t.reshape(-1))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == by * t.element_size()
    return v


class Vid:
    """One video of a table.  Host: ``planes`` float32 [n_obj * n, H, W] in UNIT order (obj * n + frame) for a float video, ``lab``
    uint8 [n, H, W] for a label video - what the reference reads.  Device: the masks in one of the layouts
      dense   [n_obj, n, H, W] from a 16-byte aligned base            shift   the same, 4 bytes (labels: 1 byte) later
      allp    all_P [n, n_obj + 1, H, W], plane 0 junk: frame stride (n_obj + 1) * H * W, object stride H * W (object-major units)."""

    def __init__(self, dev, H, W, n, O, planes=None, lab=None, layout="dense", u8=False, frames=None):
        self.H, self.W, self.n, self.O, self.u8 = H, W, n, O, u8
        self.units, self.plane = n * O, H * W
        self.planes, self.lab = planes, lab
        self.is_lab = lab is not None
        self._ref = None
        if frames is None:                                                       # the box and delta entries never read the frames
            frames = torch.zeros(4, dtype=torch.float32, device=dev)
        self.frames = frames
        if self.is_lab:
            assert lab.shape == (n, H, W) and lab.dtype == np.uint8
            d = torch.from_numpy(lab).to(dev)
            self.d = d if layout == "dense" else _shifted(d)
            self.stride_frame, self.stride_obj = self.plane, 0
        else:
            assert planes.shape == (n * O, H, W) and planes.dtype == np.float32
            if layout == "allp":
                allp = np.random.RandomState(n * O).rand(n, O + 1, H, W).astype(np.float32)
                for o in range(O):
                    for f in range(n):
                        allp[f, o + 1] = planes[o * n + f]
                self.all_p = torch.from_numpy(allp).to(dev)
                self.d = self.all_p[:, 1:]
                self.stride_frame, self.stride_obj = (O + 1) * self.plane, self.plane
            else:
                d = torch.from_numpy(planes).to(dev)
                self.d = d if layout == "dense" else _shifted(d)
                self.stride_frame, self.stride_obj = self.plane, n * self.plane
        self.vec = (self.d.data_ptr() % 16 == 0) and self.plane % (16 if self.is_lab else 4) == 0

    @classmethod
    def on(cls, d, H, W, n, O, stride_frame, stride_obj):
        """A float video on masks that are already on the device (d: its first plane), with the given strides in elements."""
        v = cls.__new__(cls)
        v.H, v.W, v.n, v.O, v.u8, v.units, v.plane, v.is_lab = H, W, n, O, False, n * O, H * W, False
        v.frames, v.d, v.stride_frame, v.stride_obj, v.planes, v.lab = d, d, stride_frame, stride_obj, None, None
        return v

    def desc(self):
        kind = L.FRAMES_RGBX8 if self.u8 else L.FRAMES_F32
        if self.is_lab:
            return L.Video(self.frames.data_ptr(), None, 0, 0, kind, self.n, self.O, self.H, self.W)
        return L.Video(self.frames.data_ptr(), self.d.data_ptr(), self.stride_frame, self.stride_obj, kind, self.n, self.O, self.H, self.W)

    def labels(self):
        return L.Labels(self.d.data_ptr(), self.stride_frame) if self.is_lab else L.Labels(None, 0)

    def ref(self):
        """(bbox_ref, bbox_minmax_ref) of the video's units, computed once (a label video: on its one-hot planes)."""
        if self._ref is None:
            if not self.is_lab:
                self._ref = (fr.bbox_ref(self.planes), fr.bbox_minmax_ref(self.planes))
            else:
                p = fr.label_planes(self.lab, self.O)
                self._ref = (fr.bbox_ref(p), fr.bbox_minmax_ref(p))
        return self._ref


def _arrays(vids):
    arr = (L.Video * len(vids))(*[v.desc() for v in vids])
    lab = (L.Labels * len(vids))(*[v.labels() for v in vids]) if any(v.is_lab for v in vids) else None
    return arr, lab


def _firsts(vids):
    return np.concatenate([[0], np.cumsum([v.units for v in vids])]).astype(np.int64)


def _bbox(dev, vids, ids=None):
    """ivosw_mask_bbox_videos(_lab) over the table, or ivosw_mask_bbox_units(_lab) over `ids` -> (yxhw, scratch) as numpy; one guard row
    behind each output, asserted untouched."""
    lib, st = L.lib(), L.stream_ptr(dev)
    arr, lab = _arrays(vids)
    B = int(_firsts(vids)[-1]) if ids is None else len(ids)
    out = torch.full((B + 1, 4), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.full((B + 1, 4), SENT, dtype=torch.int32, device=dev)
    if ids is None:
        if lab is None:
            L.check(lib.ivosw_mask_bbox_videos(arr, len(vids), L.dptr(out), L.dptr(scratch), st), "mask_bbox_videos")
        else:
            L.check(lib.ivosw_mask_bbox_videos_lab(arr, lab, len(vids), L.dptr(out), L.dptr(scratch), st), "mask_bbox_videos_lab")
    else:
        d_ids = torch.tensor(list(ids), dtype=torch.int32, device=dev)
        if lab is None:
            L.check(lib.ivosw_mask_bbox_units(arr, len(vids), L.dptr(d_ids), B, L.dptr(out), L.dptr(scratch), st), "mask_bbox_units")
        else:
            L.check(lib.ivosw_mask_bbox_units_lab(arr, lab, len(vids), L.dptr(d_ids), B, L.dptr(out), L.dptr(scratch), st), "mask_bbox_units_lab")
    o, s = out.cpu().numpy(), scratch.cpu().numpy()
    assert np.isnan(o[B]).all() and (s[B] == SENT).all(), "the guard row behind the outputs was written"
    return o[:B], s[:B]


def _table_ref(vids):
    """The table's reference in unit order first[v] + obj * n_frames + frame, written out."""
    first = _firsts(vids)
    yx, raw = np.full((first[-1], 4), np.nan, np.float32), np.full((first[-1], 4), SENT, np.int32)
    for v, f0 in zip(vids, first):
        ryx, rraw = v.ref()
        for o in range(v.O):
            for f in range(v.n):
                yx[f0 + o * v.n + f], raw[f0 + o * v.n + f] = ryx[o * v.n + f], rraw[o * v.n + f]
    return yx, raw


def _assert_table(dev, vids, why):
    yx, raw = _bbox(dev, vids)
    want_yx, want_raw = _table_ref(vids)
    np.testing.assert_array_equal(raw, want_raw, err_msg=why + ": integer box in the scratch")
    np.testing.assert_array_equal(yx, want_yx, err_msg=why)
    return yx, raw


def _groups(seq, k):
    return [seq[i:i + k] for i in range(0, len(seq), k)]


# ---------------------------------------------------------------- a. float box
def test_float_box_workload_plane_at_every_seam(dev):
    """One video of 480 x 854, 32 units or fewer per launch: S = 64, 58 chunks of 7168 = seven 1024-strides each, so the four-loads loop
    and the tail both run on carried coordinates.  Every position on either side of every seam and the plane's ends is the lone pixel of
    some unit (the pixel before a seam is met on the chunk's seventh visit); a sparse plane rides along."""
    H, W = 480, 854
    chunk, pos = fr.lone_positions(H, W, 32, strides=False)
    assert chunk == 7168 and len(pos) >= 2 * 57 + 3
    sparse = fr.sparse_plane(np.random.RandomState(11), H, W)[None]
    for g, group in enumerate(_groups(pos, 31)):
        planes = np.concatenate([fr.lone_planes(H, W, group), sparse])
        n_units = len(planes)
        assert n_units <= 32 and fr.scan_seams_multi([H * W], n_units)[0] == 7168
        O = 2 if n_units % 2 == 0 else 1
        for layout in ("dense", "shift"):
            v = Vid(dev, H, W, n_units // O, O, planes, layout=layout)
            assert v.vec == (layout == "dense")
            _assert_table(dev, [v], f"launch {g}, {layout}")


def test_float_box_carried_coordinates(dev):
    """70 x 1100 and 80 x 1024 in one table of 32 units: chunk 2048, the second visit of every workgroup is carried with sy = 0 (W > 1024)
    and sx = 0 (W = 1024).  Lone pixels on both sides of every seam and every stride."""
    sizes = fr.MULTI_CARRY_SIZES
    todo = []
    for H, W in sizes:
        chunk, pos = fr.lone_positions(H, W, 32)
        assert chunk == 2048 and {2047, 2048, 1023, 1024, 1027, 3071, 3072} <= set(pos)
        todo.append(_groups(pos, 16))
    assert fr.scan_seams_multi([H * W for H, W in sizes], 32)[0] == 2048
    rs = np.random.RandomState(5)
    for g in range(max(len(t) for t in todo)):
        for layout in ("dense", "shift"):
            vids = []
            for (H, W), groups in zip(sizes, todo):
                group = groups[g] if g < len(groups) else []
                planes = np.concatenate([fr.lone_planes(H, W, group)] + [fr.sparse_plane(rs, H, W)[None] for _ in range(16 - len(group))])
                vids.append(Vid(dev, H, W, 8, 2, planes, layout=layout))
            assert sum(v.units for v in vids) == 32
            _assert_table(dev, vids, f"launch {g}, {layout}")


def _one_chunk_vids(dev, layout):
    """More than 2048 units over five videos of one table: S = 1, every unit's plane is ONE workgroup's range.  Per video: a full, an
    empty and random sparse planes, and in its LAST units a lone pixel at each of stride_edges."""
    vids = []
    for k, (H, W) in enumerate(fr.ONE_CHUNK_SIZES):
        n, O = (683, 3) if (H, W) == (8, 8) else (150, 3)
        rs = np.random.RandomState(2049 + W)
        planes = np.where(rs.rand(n * O, H, W) < 2.0 / (H * W), 0.9, 0.1 * rs.rand(n * O, H, W)).astype(np.float32)
        planes[0], planes[1] = 1.0, 0.0
        pos = fr.stride_edges(H, W)
        assert len(pos) + 2 < n * O and (H * W <= 1024 or {1023, 1024, 1027} <= set(pos))
        planes[n * O - len(pos):] = fr.lone_planes(H, W, pos)
        vids.append(Vid(dev, H, W, n, O, planes, layout=layout))
    units = sum(v.units for v in vids)
    chunk, seams = fr.scan_seams_multi([v.plane for v in vids], units)
    assert units == 4 * 450 + 2049 and chunk == 5120 and all(s == [] for s in seams)
    return vids


@pytest.fixture(scope="module")
def one_chunk_tables(dev):
    return {layout: _one_chunk_vids(dev, layout) for layout in ("dense", "shift")}


def test_float_box_one_chunk_per_unit(dev, one_chunk_tables):
    """grid (1, 3849).  4 x 1024 and 2048 x 2 (sy = 512: a float4 spans two rows) run the four-loads loop in every lane, 4 x 1025 and
    4 x 1100 the loop and the tail; 8 x 8 leaves most lanes without work."""
    for layout, vids in one_chunk_tables.items():
        assert all(v.vec == (layout == "dense") for v in vids)
        _, raw = _assert_table(dev, vids, layout)
        assert len(np.unique(raw, axis=0)) > 300


def _mixed_vids(dev):
    """Eight videos, 42 units: the chunk (9216) is set by the 480 x 854 plane, which holds ONE unit; every other video's workgroups behind
    its own plane leave early.  70 x 1100 takes a lone pixel on each side of every seam that falls inside ITS plane; the others random
    sparse planes with lone pixels at their ends."""
    rs = np.random.RandomState(42)
    spec = [(480, 854, 1, 1, "dense"), (70, 1100, 11, 2, "dense"), (37, 53, 2, 2, "dense"), (2, 2, 3, 1, "dense"), (8, 2, 1, 2, "dense"),
            (6, 300, 2, 1, "dense"), (16, 24, 3, 2, "allp"), (12, 20, 2, 1, "shift")]
    units = sum(n * O for _, _, n, O, _ in spec)
    chunk, seams = fr.scan_seams_multi([H * W for H, W, _, _, _ in spec], units)
    assert units == 42 and chunk == 9216 and len(seams[0]) == 44 and len(seams[1]) == 8 and all(s == [] for s in seams[2:])
    vids = []
    for (H, W, n, O, layout), sm in zip(spec, seams):
        planes = np.stack([fr.sparse_plane(rs, H, W) for _ in range(n * O)])
        if (H, W) == (70, 1100):
            pos = sorted({p for s in sm for p in (s - 1, s)} | {0, H * W - 1, H * W - 4})
            planes[:len(pos)] = fr.lone_planes(H, W, pos)
        elif n * O >= 2:
            planes[-2:] = fr.lone_planes(H, W, [0, H * W - 1])
        vids.append(Vid(dev, H, W, n, O, planes, layout=layout))
    assert [v.vec for v in vids] == [True, True, False, True, True, True, True, False]
    return vids


@pytest.fixture(scope="module")
def mixed_table(dev):
    return _mixed_vids(dev)


def test_float_box_mixed_table(dev, mixed_table):
    """Unit order first[v] + obj * n_frames + frame across eight videos of eight sizes, an object-major strided all_P and a misaligned
    base among them (_table_ref writes that order out)."""
    _, raw = _assert_table(dev, mixed_table, "mixed table")
    assert len(np.unique(raw, axis=0)) >= 30


# ---------------------------------------------------------------- b. label box
def _lone_label_vids(dev, H, W, n, O, positions, layout):
    """n frames x O objects, every object the lone pixel of one position per frame (the last frame may hold fewer: empty planes)."""
    per = _groups(positions, O) + [[] for _ in range(n)]
    lab = np.stack([fr.lone_label_map(H, W, per[f]) for f in range(n)])
    return Vid(dev, H, W, n, O, lab=lab, layout=layout)


@pytest.mark.parametrize("B", [32, 128])
def test_label_box_workload_plane(dev, B):
    """480 x 854 label maps, 16 pixels per lane, block stride 4096.  B = 32 units: chunk 7168, one carried visit in the tail loop;
    B = 128 units: chunk 26624, the 4 x 4096 loop carries three times and the tail twice more.  A lone label on both sides of every seam
    and every stride inside a chunk, at the end of the vector that starts at a stride, and at the plane's ends; from an aligned base
    (vector scan) and one byte later (byte scan)."""
    H, W = 480, 854
    chunk, pos = fr.lone_positions(H, W, B, label=True)
    assert chunk == {32: 7168, 128: 26624}[B] and fr.scan_seams_multi([H * W], B)[0] == chunk
    n, O = (2, 16) if B == 32 else (1, 128)
    for g, group in enumerate(_groups(pos, B)):
        ref = None
        for layout in ("dense", "shift"):
            v = _lone_label_vids(dev, H, W, n, O, group, layout)
            assert v.units == B and v.vec == (layout == "dense")
            if ref is not None:
                v._ref = ref                                                     # the same maps: the reference is computed once
            _, raw = _assert_table(dev, [v], f"launch {g}, {layout}")
            ref = v._ref
            assert int((raw[:, 1] >= 0).sum()) == len(group) and (raw[:, 0] == raw[:, 1])[raw[:, 1] >= 0].all()


def _label_one_chunk_vids(dev, layout):
    """2295 units (S = 1) on 16 x 1100 (5 frames) and 16 x 1024 (4 frames), n_obj = 255, plus 37 x 53 (odd plane: byte scan).  Labels
    1 .. len(stride_edges) are lone pixels at stride_edges (another assignment per frame), 18 .. 255 scattered at random."""
    vids = []
    for (H, W), n in zip(fr.LABEL_ONE_CHUNK_SIZES + ((37, 53),), (5, 4, 2)):
        rs = np.random.RandomState(H * W)
        pos = fr.stride_edges(H, W, 4096, 16)
        O = 255 if W >= 1024 else 3
        lab = np.where(rs.rand(n, H * W) < 0.01, rs.randint(len(pos) + 1 if O == 255 else 1, 256, (n, H * W)), 0).astype(np.uint8)
        if O == 255:
            assert {4095, 4096, 4111, 12287, 12288, H * W - 16, H * W - 1} <= set(pos)
            for f in range(n):
                lab[f, pos] = 1 + (np.arange(len(pos)) + 5 * f) % len(pos)
        vids.append(Vid(dev, H, W, n, O, lab=lab.reshape(n, H, W), layout=layout))
    units = sum(v.units for v in vids)
    assert units == 1275 + 1020 + 6 and fr.scan_seams_multi([v.plane for v in vids], units) == (18432, [[], [], []])
    return vids


@pytest.fixture(scope="module")
def label_one_chunk_tables(dev):
    return {layout: _label_one_chunk_vids(dev, layout) for layout in ("dense", "shift")}


def test_label_box_one_chunk_per_unit(dev, label_one_chunk_tables):
    for layout, vids in label_one_chunk_tables.items():
        assert [v.vec for v in vids] == [layout == "dense", layout == "dense", False]
        _, raw = _assert_table(dev, vids, layout)
        assert len(np.unique(raw, axis=0)) > 300


def test_label_box_hard_byte_values(dev):
    """fr.hard_byte_map: every label 1 .. 255 next to label ^ 0x80, label - 1, label + 1, 0 and 255 inside one 32-bit word, and a word of
    those neighbours without it; read with n_obj = 255 and, from the same map, with n_obj = 100 (values above belong to no unit)."""
    m = fr.hard_byte_map()
    for layout in ("dense", "shift"):
        vids = [Vid(dev, 16, 256, 5, 255, lab=m, layout=layout), Vid(dev, 16, 256, 5, 100, lab=m, layout=layout)]
        assert all(v.vec == (layout == "dense") for v in vids)
        _, raw = _assert_table(dev, vids, layout)
        for f, lab in fr.hard_byte_units():
            at = 16 * lab + 4 * ((lab >> 1) & 1)
            np.testing.assert_array_equal(raw[(lab - 1) * 5 + f], [at // 256, at // 256, at % 256 + 1, at % 256 + 4])


def _label_mixed_vids(dev):
    """A float video, a label video on fp32 frames and a label video on RGBX8 frames (35 units); the maps hold 0 .. n_obj + 1 and 255."""
    rs = np.random.RandomState(8)
    P = np.stack([fr.sparse_plane(rs, 24, 36) for _ in range(4)])
    la = rs.choice(np.array([0, 0, 0, 1, 2, 3, 4, 255], np.uint8), (3, 40, 64), p=[0.3, 0.3, 0.33, 0.02, 0.02, 0.01, 0.01, 0.01])
    la[0][la[0] == 2] = 0                                                        # object 2 absent from frame 0: the empty box
    lb = rs.choice(np.array([0, 1, 2, 3, 255], np.uint8), (11, 37, 53), p=[0.96, 0.01, 0.01, 0.01, 0.01])
    rgbx = torch.zeros(4, dtype=torch.uint8, device=dev)
    return [Vid(dev, 24, 36, 2, 2, P), Vid(dev, 40, 64, 3, 3, lab=la), Vid(dev, 37, 53, 11, 2, lab=lb, u8=True, frames=rgbx)]


@pytest.fixture(scope="module")
def label_mixed_table(dev):
    return _label_mixed_vids(dev)


def test_label_box_mixed_table(dev, label_mixed_table):
    assert sum(v.units for v in label_mixed_table) == 35
    _, raw = _assert_table(dev, label_mixed_table, "float + label + RGBX8 label")
    assert (raw[4 + 3] == [np.iinfo(np.int32).max, -1, np.iinfo(np.int32).max, -1]).all()


# ---------------------------------------------------------------- c. unit lists
def _check_unit_lists(dev, vids, sizes, seed):
    """ivosw_mask_bbox_units(_lab): a permuted list with repeated ids, -1 and `units` in it.  Each row bit equal to the row of the range
    entry for that id and equal to the reference; the rows of the two ids outside the table all zero."""
    units = int(_firsts(vids)[-1])
    all_yx, all_raw = _bbox(dev, vids)
    want_yx, want_raw = _table_ref(vids)
    rs = np.random.RandomState(seed)
    for n_ids in sizes:
        assert n_ids <= units
        ids = rs.permutation(units)[:n_ids] if n_ids < units // 2 else rs.randint(0, units, n_ids)
        ids = ids.astype(np.int64)
        if n_ids >= 8:
            ids[3], ids[5], ids[1], ids[n_ids - 1] = ids[0], ids[0], -1, units   # a repeated id, and the two ids outside the table
        yx, raw = _bbox(dev, vids, ids.tolist())
        ok = (ids >= 0) & (ids < units)
        assert ok.sum() >= n_ids - 2
        np.testing.assert_array_equal(yx[ok].view(np.int32), all_yx[ids[ok]].view(np.int32), err_msg=f"n_ids = {n_ids}")
        np.testing.assert_array_equal(raw[ok], all_raw[ids[ok]], err_msg=f"n_ids = {n_ids}")
        np.testing.assert_array_equal(yx[ok], want_yx[ids[ok]], err_msg=f"n_ids = {n_ids}")
        np.testing.assert_array_equal(raw[ok], want_raw[ids[ok]], err_msg=f"n_ids = {n_ids}")
        assert (yx[~ok].view(np.int32) == 0).all()


def test_unit_lists_on_the_one_chunk_table(dev, one_chunk_tables):
    """The range entry runs S = 1 (3849 units); a list of 1 or 33 ids runs S = 5 chunks of 1024 on the same planes, one of 2100 S = 1."""
    for layout, vids in one_chunk_tables.items():
        _check_unit_lists(dev, vids, (1, 33, 2100), seed=1)


def test_unit_lists_on_the_mixed_table(dev, mixed_table):
    """n_ids = 1: chunk 7168 (the list entry sizes its grid for the largest plane of the table whatever it names), 33: 7168, against 9216."""
    _check_unit_lists(dev, mixed_table, (1, 33, 42), seed=2)


def test_unit_lists_on_the_label_tables(dev, label_one_chunk_tables, label_mixed_table):
    for layout, vids in label_one_chunk_tables.items():
        _check_unit_lists(dev, vids, (1, 33, 2100), seed=3)
    _check_unit_lists(dev, label_mixed_table, (1, 33), seed=4)


# ---------------------------------------------------------------- d. delta and compaction
class Delta:
    """flags | guard | unit_ids | guard | n_dirty | guard in one buffer; run() -> the dirty list, guards asserted."""

    def __init__(self, dev, vids, caches):
        self.dev, self.vids, self.caches = dev, vids, caches
        self.units = int(_firsts(vids)[-1])

    def run(self, cold):
        lib, U = L.lib(), self.units
        meta = torch.full((2 * U + 3,), SENT, dtype=torch.int32, device=self.dev)
        flags, ids, n = meta[:U], meta[U + 1:2 * U + 1], meta[2 * U + 2:2 * U + 3]
        arr, lab = _arrays(self.vids)
        ptrs = (ctypes.c_void_p * len(self.caches))(*[c.data_ptr() for c in self.caches])
        args = (ptrs, L.int_array(cold), L.dptr(flags), L.dptr(ids), L.dptr(n), L.stream_ptr(self.dev))
        if lab is None:
            L.check(lib.ivosw_mask_delta_videos(arr, len(self.vids), *args), "mask_delta_videos")
        else:
            L.check(lib.ivosw_mask_delta_videos_lab(arr, lab, len(self.vids), *args), "mask_delta_videos_lab")
        h = meta.cpu().numpy()
        assert h[U] == SENT and h[2 * U + 1] == SENT, "a guard between the outputs was written"
        nd = int(h[2 * U + 2])
        assert 0 <= nd <= U, nd
        return h[U + 1:U + 1 + nd].copy()                                        # the entries behind n_dirty are unspecified: not looked at


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2048, 2049, 3001])
def test_delta_compaction_beyond_one_round(dev, N):
    """N units of 2 x 2 planes over 32 videos: delta_compact_kernel walks the flags 1024 at a time and carries its total.  On the float4
    compare (aligned planes and cache) and on the scalar one (both 4 bytes later)."""
    rs = np.random.RandomState(N)
    share = [N // 32 + (1 if i < N % 32 else 0) for i in range(32)]
    for shift in (0, 1):
        planes = _shifted(torch.from_numpy(rs.rand(N, 4).astype(np.float32)).to(dev), shift).view(N, 4)
        cache = _shifted(torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31 - 1, (N, 4)).astype(np.int32)).to(dev), shift).view(N, 4)
        vids, caches, first = [], [], 0
        for i, u in enumerate(share):
            O = 2 if (u % 2 == 0 and i % 3 == 0) else 1
            vids.append(Vid.on(planes[first:], 2, 2, u // O, O, 4, (u // O) * 4))
            caches.append(cache[first:].view(torch.float32))
            first += u
        assert first == N
        D = Delta(dev, vids, caches)
        patterns = [("cold", np.arange(N)), ("none", np.arange(0)), ("unit 0", np.array([0])), ("the last unit", np.array([N - 1])),
                    ("1023 and 1024", np.array([u for u in (1023, 1024) if u < N], np.int64)), ("a random half", np.flatnonzero(rs.rand(N) < 0.5))]
        for name, dirty in patterns:
            expected = np.zeros(N, bool)
            expected[dirty] = True
            if name != "cold" and dirty.size:
                idx = torch.from_numpy(dirty).to(dev)
                planes[idx, torch.from_numpy(dirty % 4).to(dev)] += 1.0
            got = D.run([1 if name == "cold" else 0] * 32)
            np.testing.assert_array_equal(got, np.flatnonzero(expected), err_msg=f"{name}, shift {shift}")
            assert torch.equal(cache, planes.view(torch.int32)), (name, shift)


@pytest.mark.parametrize("H,W", [(480, 854), (130, 128), (131, 127)])
def test_label_delta_beyond_one_slice(dev, H, W):
    """n_obj = 70, two frames.  480 x 854: 26 slices of 16384 bytes, the last one 320; 130 x 128: a second slice of 256 bytes; 131 x 127
    (H * W % 16 = 13): the byte compare.  Single-byte edits at the first and last byte of every slice, on both sides of every 4096 stride
    of the first slice and at the plane's last byte; per position the byte is first forced to a, then goes a -> b, over: two labels
    <= 64, a label > 64 (the plain-store path), 0 <-> n_obj + 1 (nothing dirty), 70 -> 64, 200 -> 1."""
    n, O, plane = 2, 70, H * W
    assert (plane % 16 == 0) == (W != 127)
    slices = list(range(0, plane, 16384))
    assert len(slices) == {854: 26, 128: 2, 127: 2}[W] and plane - slices[-1] == {854: 320, 128: 256, 127: 253}[W]
    rs = np.random.RandomState(W)
    host = rs.choice(np.array([0, 1, 2, 3, 64, 65, 70, 71, 200], np.uint8), (n, H, W))
    v = Vid(dev, H, W, n, O, lab=host.copy())
    cache = torch.from_numpy(rs.randint(0, 256, (n, H, W)).astype(np.uint8)).to(dev)
    assert cache.data_ptr() % 16 == 0
    D = Delta(dev, [v], [cache])
    np.testing.assert_array_equal(D.run([1]), np.arange(n * O))                  # cold: every unit, the map is copied
    assert torch.equal(cache, v.d)
    assert D.run([0]).size == 0                                                  # unchanged
    pos = sorted({p for s in slices for p in (s, min(plane, s + 16384) - 1)} | {s + d for s in (4096, 8192, 12288) for d in (-1, 0)} | {plane - 1})
    kinds = [(1, 2), (3, 65), (0, 71), (71, 0), (70, 64), (200, 1)]
    new = host.copy()
    for k, p in enumerate(pos):
        f = k % n
        for value in kinds[k % len(kinds)]:
            new.reshape(n, plane)[f, p] = value
            v.d.view(n, plane)[f, p] = value
            want = fr.label_delta_ref(host, new, O)
            if (value, k % len(kinds)) in ((71, 2), (0, 3)) and host.reshape(n, plane)[f, p] in (0, 71):
                assert want == []
            np.testing.assert_array_equal(D.run([0]), want, err_msg=f"byte {p} of frame {f} -> {value}")
            assert torch.equal(cache, v.d), (p, f, value)
            host.reshape(n, plane)[f, p] = value
    assert D.run([0]).size == 0


def test_delta_table_label_float_label(dev):
    """label (2 frames x 3 objects, vector compare), float (3 frames x 2 objects), label (4 frames x 2 objects, 37 x 53: byte compare): the
    label compare finds its video by ffirst = 0, 2, 2 and the float compare skips the label units; one edit in each video."""
    rs = np.random.RandomState(12)
    la = rs.randint(0, 5, (2, 20, 16)).astype(np.uint8)
    P = rs.rand(6, 10, 12).astype(np.float32)
    lb = rs.randint(0, 4, (4, 37, 53)).astype(np.uint8)
    vids = [Vid(dev, 20, 16, 2, 3, lab=la.copy()), Vid(dev, 10, 12, 3, 2, P.copy()), Vid(dev, 37, 53, 4, 2, lab=lb.copy())]
    caches = [torch.full((2 * 320,), 9, dtype=torch.uint8, device=dev), torch.full((6 * 120,), 9.0, dtype=torch.float32, device=dev),
              torch.full((4 * 1961,), 9, dtype=torch.uint8, device=dev)]
    first = _firsts(vids)
    assert first.tolist() == [0, 6, 12, 20]
    D = Delta(dev, vids, caches)

    def settled():
        return all(torch.equal(c.view(-1), v.d.reshape(-1).view(c.dtype)) for c, v in zip(caches, vids))
    np.testing.assert_array_equal(D.run([1, 1, 1]), np.arange(20))
    assert settled() and D.run([0, 0, 0]).size == 0
    na, nb = la.copy(), lb.copy()
    na[1, 19, 15] = na[1, 19, 15] % 3 + 1                                        # labels 1 .. 3 only: both units of the pixel exist
    nb[3, 36, 52] = 2 if lb[3, 36, 52] != 2 else 1                               # the last byte of the last frame of the last video
    vids[0].d[1, 19, 15], vids[2].d[3, 36, 52] = int(na[1, 19, 15]), int(nb[3, 36, 52])
    vids[1].d[1 * 3 + 2, 9, 11] += 0.5                                           # unit obj 1, frame 2 of the float video
    want = [int(first[0]) + u for u in fr.label_delta_ref(la, na, 3)] + [int(first[1]) + 5] + [int(first[2]) + u for u in fr.label_delta_ref(lb, nb, 2)]
    assert len(want) >= 3
    np.testing.assert_array_equal(D.run([0, 0, 0]), want)
    assert settled() and D.run([0, 0, 0]).size == 0
    for f in range(4):                                                           # every frame of the second label video on its own
        old = nb.copy()
        nb[f, 0, f] = 1 if nb[f, 0, f] != 1 else 2
        vids[2].d[f, 0, f] = int(nb[f, 0, f])
        np.testing.assert_array_equal(D.run([0, 0, 0]), [int(first[2]) + u for u in fr.label_delta_ref(old, nb, 2)], err_msg=f"frame {f}")
        assert settled()
    np.testing.assert_array_equal(D.run([0, 1, 0]), np.arange(6, 12))            # the float video alone cold


# ---------------------------------------------------------------- e. sampler at workload size
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _single(dev, v, tp_units, boxes, dt, tdt):
    """ivosw_roi_sample / ivosw_roi_sample_u8 on the video's units materialised: the frames repeated per unit, the planes contiguous."""
    fidx = torch.arange(v.units, device=dev) % v.n
    tf = v.frames[fidx].contiguous()
    roi = torch.empty(v.units, 256, 256, 4, dtype=tdt, device=dev)
    fn = L.lib().ivosw_roi_sample_u8 if v.u8 else L.lib().ivosw_roi_sample
    L.check(fn(L.dptr(tf), L.dptr(tp_units), L.dptr(boxes), v.units, v.H, v.W, dt, L.dptr(roi), L.stream_ptr(dev)), "roi_sample")
    return roi


@pytest.mark.parametrize("kinds", [("f32", "u8"), ("u8", "f32")], ids=["f32+u8", "u8+f32"])
def test_sampler_at_workload_size(dev, kinds):
    """480 x 854 (3 frames x 2 objects) and 150 x 200 (2 frames x 3 objects) in one table, the six fr.border_boxes of each size: boxes over
    every frame border AND inside the frame, which frames of 56 pixels never allow.  ivosw_roi_sample_videos, _units (a permuted list with
    a repeat and a -1) and _videos_lab (label maps) bit equal to the single-video sampler on the materialised planes, fp32 and bf16."""
    lib, st = L.lib(), L.stream_ptr(dev)
    g = torch.Generator().manual_seed(854)
    rs = np.random.RandomState(854)
    fvids, lvids, boxes = [], [], []
    for (H, W, n, O), kind in zip(((480, 854, 3, 2), (150, 200, 2, 3)), kinds):
        if kind == "u8":
            frames = torch.randint(0, 256, (n, H, W, 4), generator=g, dtype=torch.uint8)
            frames[..., 3] = 0
        else:
            frames = torch.rand(n, 3, H, W, generator=g)
        frames = frames.to(dev)
        planes = (0.1 * rs.rand(n * O, H, W)).astype(np.float32)
        lab = np.zeros((n, H, W), np.uint8)
        for u in range(n * O):
            y0, x0 = rs.randint(0, H // 2), rs.randint(0, W // 2)
            planes[u, y0:y0 + rs.randint(3, H // 2), x0:x0 + rs.randint(3, W // 2)] = 0.9
            lab[u % n, y0:y0 + rs.randint(3, H // 2), x0:x0 + rs.randint(3, W // 2)] = u // n + 1
        lab[:, 0, :5] = O + 1                                                    # a label nobody owns
        fvids.append(Vid(dev, H, W, n, O, planes, u8=(kind == "u8"), frames=frames))
        lvids.append(Vid(dev, H, W, n, O, lab=lab, u8=(kind == "u8"), frames=frames))
        boxes.append(fr.border_boxes(H, W)[np.arange(n * O) % 6])
    units = 12
    d_box = torch.from_numpy(np.concatenate(boxes)).to(dev)
    order = [7, 0, 11, 3, -1, 5, 0, 9, 2, 6]
    d_ids = torch.tensor(order, dtype=torch.int32, device=dev)
    inside = [i for i, u in enumerate(order) if u >= 0]
    for name, (dt, tdt) in DT.items():
        for vids, what in ((fvids, "float masks"), (lvids, "label maps")):
            want = torch.cat([_single(dev, v, torch.from_numpy(v.planes if not v.is_lab else fr.label_planes(v.lab, v.O)).to(dev), d_box[f0:f0 + v.units], dt, tdt)
                              for v, f0 in zip(vids, _firsts(vids))])
            arr, lab = _arrays(vids)
            got = torch.full((units + 1, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
            if lab is None:
                L.check(lib.ivosw_roi_sample_videos(arr, 2, L.dptr(d_box), dt, L.dptr(got), st), "roi_sample_videos")
            else:
                L.check(lib.ivosw_roi_sample_videos_lab(arr, lab, 2, L.dptr(d_box), dt, L.dptr(got), st), "roi_sample_videos_lab")
            assert torch.equal(_bits(got[:units]), _bits(want)), (name, what)
            assert bool(torch.isnan(got[units].float()).all()), (name, what, "guard tile")
            p = want[..., 3].float()
            assert float(p.max()) > 0.85 and bool(((p > 0.2) & (p < 0.8)).any())                 # the mask channel is there, and interpolated
            lbox = d_box[[max(u, 0) for u in order]].contiguous()
            gl = torch.full((len(order) + 1, 256, 256, 4), float("nan"), dtype=tdt, device=dev)
            if lab is None:
                L.check(lib.ivosw_roi_sample_units(arr, 2, L.dptr(d_ids), len(order), L.dptr(lbox), dt, L.dptr(gl), st), "roi_sample_units")
            else:
                L.check(lib.ivosw_roi_sample_units_lab(arr, lab, 2, L.dptr(d_ids), len(order), L.dptr(lbox), dt, L.dptr(gl), st), "roi_sample_units_lab")
            assert torch.equal(_bits(gl[inside]), _bits(want[[order[i] for i in inside]])), (name, what, "unit list")
            assert bool((_bits(gl[4]) == 0).all()) and bool(torch.isnan(gl[len(order)].float()).all()), (name, what)
