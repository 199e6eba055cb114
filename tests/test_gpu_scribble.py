"""GPU: the scribble rasteriser and rough_ROI (csrc/scribble.hip) through the C ABI and through their host functions against the numpy
definition of tests/scribble_ref.py and the recorded reference function (tests/golden/scribble_fixtures.npz), every comparison bit for
bit: the work is integer work and the float planes hold small integers.

Every buffer, the workspace included, lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.
Odd sizes and one-element pointer offsets take the element-by-element kernels, 16-byte aligned buffers the vector ones."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import scribbles as S
from tests import scribble_ref as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scribble_fixtures.npz")
PAD = 16                                                  # elements in front of and behind every buffer
I8_FILL, F32_FILL, WS_FILL = 77, 77.5, 0xAB
ERR_ARG, ERR_WS = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _vector_path(monkeypatch):
    monkeypatch.delenv("IVOSW_SCRIBBLE_SCALAR", raising=False)


class Buf:
    """A device buffer holding `data` (flat) PAD + off elements inside an allocation filled with `fill`; `back()` returns the data as
    it is now after checking the guard bands."""

    def __init__(self, dev, data, fill, off=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.lo, self.n = PAD + off, data.size
        self.host = np.full(data.size + 3 * PAD, fill, data.dtype)
        self.host[self.lo:self.lo + self.n] = data
        self.t = torch.from_numpy(self.host).to(dev)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.lo * self.t.element_size())

    def back(self, name, unchanged=False):
        h = self.t.cpu().numpy()
        bits = lambda a: a.view(np.uint8)
        assert (bits(h[:self.lo]) == bits(self.host[:self.lo])).all() and (bits(h[self.lo + self.n:]) == bits(self.host[self.lo + self.n:])).all(), \
            f"{name}: written outside its extent"
        if unchanged:
            np.testing.assert_array_equal(bits(h), bits(self.host), err_msg=f"{name}: written by a refused call / an input")
        return h[self.lo:self.lo + self.n]


class Call:
    """One ivosw_scribble_raster call with every buffer in guard bands; keyword overrides replace single C arguments."""

    def __init__(self, dev, points, table, n_maps, H, W, off=0, want=("i8", "f32")):
        self.points = np.asarray(points, np.int32).reshape(-1, 2)
        self.table = np.ascontiguousarray(np.asarray(table, np.int32).reshape(-1, 4))
        self.shape = (n_maps, H, W)
        n = max(n_maps * H * W, 1)
        self.b_points = Buf(dev, self.points if len(self.points) else np.zeros(2, np.int32), -7)
        self.b_table = Buf(dev, self.table if len(self.table) else np.zeros(4, np.int32), -7)
        self.b_i8 = Buf(dev, np.full(n, I8_FILL, np.int8), I8_FILL, off) if "i8" in want else None
        self.b_f32 = Buf(dev, np.full(n, F32_FILL, np.float32), F32_FILL, off) if "f32" in want else None
        self.need = L.lib().ivosw_scribble_raster_ws_bytes(max(n_maps, 1), max(H, 1), max(W, 1))
        self.b_ws = Buf(dev, np.full(max(self.need, 16), WS_FILL, np.uint8), WS_FILL)
        self.dev = dev

    def run(self, default=-1, bresenham=1, roi=-1, **over):
        n_maps, H, W = self.shape
        n_paths = len(self.table)
        a = dict(points=self.b_points.ptr() if n_paths else None, n_points=len(self.points), paths=self.b_table.ptr() if n_paths else None,
                 paths_host=self.table.ctypes.data if n_paths else None, n_paths=n_paths, n_maps=n_maps, H=H, W=W, default=default,
                 bresenham=bresenham, roi=roi, out_i8=self.b_i8.ptr() if self.b_i8 else None, out_f32=self.b_f32.ptr() if self.b_f32 else None,
                 ws=self.b_ws.ptr(), ws_bytes=self.need)
        a.update(over)
        return L.lib().ivosw_scribble_raster(a["points"], a["n_points"], a["paths"], a["paths_host"], a["n_paths"], a["n_maps"], a["H"], a["W"],
                                             a["default"], a["bresenham"], a["roi"], a["out_i8"], a["out_f32"], a["ws"], a["ws_bytes"],
                                             L.stream_ptr(self.dev))

    def outputs(self, unchanged=False):
        """(int8 map, float map) after the guard bands of EVERY buffer were checked; inputs must be as they were."""
        self.b_points.back("points", unchanged=True)
        self.b_table.back("paths", unchanged=True)
        self.b_ws.back("ws", unchanged=unchanged)
        i8 = self.b_i8.back("out_i8", unchanged).reshape(self.shape) if self.b_i8 else None
        f32 = self.b_f32.back("out_f32", unchanged).reshape(self.shape) if self.b_f32 else None
        return i8, f32


def _check(call, want, rc):
    assert rc == 0, L.lib().ivosw_last_error()
    i8, f32 = call.outputs()
    if i8 is not None:
        np.testing.assert_array_equal(i8, want)
    if f32 is not None:
        np.testing.assert_array_equal(f32.view(np.uint32), want.astype(np.float32).view(np.uint32))


def _table(paths, maps=None):
    """(points, table) from [(integer points, object id), ...]; ``maps``: the map index of each path (default 0)."""
    pts, rows, first = [], [], 0
    for k, (p, o) in enumerate(paths):
        pts += [list(q) for q in p]
        rows.append([first, len(p), o, 0 if maps is None else maps[k]])
        first += len(p)
    return np.array(pts, np.int32).reshape(-1, 2), np.array(rows, np.int32).reshape(-1, 4)


def _segments(H, W):
    """The segment zoo of one map size, every coordinate clipped into the map: all eight octants, dx == dy in four directions, horizontal
    and vertical both ways, zero length, a one-point path, the four borders, one corner-to-corner segment and a 1000-point random walk;
    object ids run through 0 .. 126 with 0 and 126 among them."""
    cx, cy = W // 2, H // 2
    clip = lambda p: [(int(np.clip(x, 0, W - 1)), int(np.clip(y, 0, H - 1))) for x, y in p]
    segs = [[(cx, cy), (cx + dx, cy + dy)] for dx, dy in ((11, 4), (4, 11), (-4, 11), (-11, 4), (-11, -4), (-4, -11), (4, -11), (11, -4))]
    segs += [[(cx, cy), (cx + d, cy + e)] for d, e in ((6, 6), (-6, 6), (6, -6), (-6, -6))]
    segs += [[(1, cy), (W - 2, cy)], [(W - 2, 1), (1, 1)], [(cx, 1), (cx, H - 2)], [(2, H - 2), (2, 1)]]
    segs += [[(3, 2), (3, 2)], [(W - 1, 0)], [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1), (0, 0)], [(0, 0), (W - 1, H - 1)]]
    rng = np.random.default_rng(H * 1000 + W)
    walk = np.cumsum(np.vstack([[[cx, cy]], rng.integers(-3, 4, (999, 2))]), 0)
    segs.append([tuple(p) for p in walk])
    objs = [0, 126] + [int(v) for v in rng.integers(0, 127, len(segs))]
    return [(clip(p), objs[k]) for k, p in enumerate(segs)]


SIZES = [(1, 1), (1, 9), (9, 1), (7, 5), (33, 65), (120, 214), (480, 854)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("H,W", SIZES)
def test_raster_equals_the_definition(dev, H, W, off):
    """Two maps (one for 480 x 854): the zoo on map 0 and in reverse list order on map 1, both outputs, aligned (the 16-byte kernel with
    its scalar tail) and at a one-element offset (the element-by-element kernel)."""
    zoo = _segments(H, W)
    n_maps = 1 if H == 480 else 2
    paths, maps = list(zoo), [0] * len(zoo)
    if n_maps == 2:
        paths += zoo[::-1]
        maps += [1] * len(zoo)
    points, table = _table(paths, maps)
    want = sr.raster(points, table, n_maps, H, W)
    assert (want >= 0).any() and (n_maps == 1 or H * W < 40 or not np.array_equal(want[0], want[1]))
    call = Call(dev, points, table, n_maps, H, W, off)
    _check(call, want, call.run())
    if H == 33:                                                                       # bresenham = 0: the points alone; another default
        call = Call(dev, points, table, n_maps, H, W, off)
        want0 = sr.raster(points, table, n_maps, H, W, default_value=5, bresenham=False)
        assert (want0 == 5).sum() > (want == -1).sum()
        _check(call, want0, call.run(default=5, bresenham=0))


def test_long_segment_is_shared_by_the_lanes(dev):
    """A two-point path across 854 pixels: 14 rounds of one wave through the closed form."""
    points, table = _table([([(0, 479), (853, 0)], 3), ([(853, 470), (0, 3)], 4)])
    call = Call(dev, points, table, 1, 480, 854, want=("i8",))
    want = sr.raster(points, table, 1, 480, 854)
    one, two = sr.line_loop(0, 479, 853, 0), sr.line_loop(853, 470, 0, 3)
    assert len(one) == len(two) == 854 and (want >= 0).sum() == len(set(one) | set(two))
    _check(call, want, call.run())


def test_order_of_assignment(dev):
    H, W = 12, 13
    a, b = ([(0, 0), (12, 11)], 1), ([(12, 0), (0, 11)], 2)
    for pair in ((a, b), (b, a)):                                                     # two crossing paths, both list orders
        points, table = _table(list(pair))
        want = sr.raster(points, table, 1, H, W)
        cross = (sr.raster(*_table([a]), 1, H, W) >= 0) & (sr.raster(*_table([b]), 1, H, W) >= 0)
        assert cross.any() and (want[cross] == pair[1][1]).all()
        call = Call(dev, points, table, 1, H, W)
        _check(call, want, call.run())
    three = [([(5, 5)], 126), ([(2, 5), (9, 5)], 0), ([(5, 1), (5, 9)], 7), ([(0, 0)], 0), ([(12, 11)], 126)]        # one pixel, three paths
    points, table = _table(three)
    want = sr.raster(points, table, 1, H, W)
    assert want[0, 5, 5] == 7 and want[0, 5, 4] == 0 and want[0, 0, 0] == 0 and want[0, 11, 12] == 126
    call = Call(dev, points, table, 1, H, W)
    _check(call, want, call.run())


def test_no_paths_empty_middle_map_and_interleaved_maps(dev):
    call = Call(dev, [], [], 2, 7, 5)
    _check(call, np.full((2, 7, 5), -1, np.int8), call.run())
    call = Call(dev, [], [], 2, 7, 5)
    _check(call, np.full((2, 7, 5), 9, np.int8), call.run(default=9, n_points=0))
    paths = [([(0, 0), (8, 3)], 1), ([(8, 0), (0, 6)], 2), ([(4, 0), (4, 6)], 3), ([(0, 3), (8, 3)], 4), ([(1, 1)], 5)]
    points, table = _table(paths, maps=[0, 2, 0, 2, 0])                               # listed map-interleaved, map 1 stays empty
    want = sr.raster(points, table, 3, 7, 9)
    assert (want[1] == -1).all() and (want[0] >= 0).any() and (want[2] >= 0).any()
    for off in (0, 1):
        call = Call(dev, points, table, 3, 7, 9, off)
        _check(call, want, call.run())
    # points that no path owns (a gap in the ranges) are ignored
    table2 = table.copy()
    table2[1] = [3, 1, 2, 2]                                                          # path 1 keeps its second point only
    call = Call(dev, points, table2, 3, 7, 9)
    _check(call, sr.raster(points, table2, 3, 7, 9), call.run())


def test_the_same_call_twice_gives_identical_bytes(dev):
    zoo = _segments(33, 65)
    points, table = _table(zoo + zoo[::-1], [0] * len(zoo) + [1] * len(zoo))
    outs = []
    for _ in range(2):
        call = Call(dev, points, table, 2, 33, 65)
        assert call.run(roi=20) == 0
        outs.append(call.outputs())
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    want = sr.rough_roi(sr.raster(points, table, 2, 33, 65)[:, None].astype(np.float32))[:, 0]
    np.testing.assert_array_equal(outs[0][0], want.astype(np.int8))
    np.testing.assert_array_equal(outs[0][1].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dist", [0, 3, 20])
def test_fused_roi_where_a_lane_group_straddles_two_maps(dev, dist, off):
    """Four maps of 33 x 65 = 2145 pixels (no multiple of 16: a 16-pixel group of the vector kernel spans the end of one map and the
    start of the next and takes the second map's box there) with different boxes, one of them empty and one that ends on the last row
    and column; aligned and at a one-element offset (the element-by-element kernel)."""
    H, W = 33, 65
    paths = [([(2, 1), (9, 4)], 1), ([(40, 20), (64, 32)], 2), ([(64, 32)], 3), ([(0, 0), (5, 0)], 126), ([(30, 30), (3, 8), (20, 2)], 0)]
    points, table = _table(paths, [0, 1, 1, 3, 3])                                    # map 2 stays empty
    drawn = sr.raster(points, table, 4, H, W)
    want = sr.rough_roi(drawn[:, None].astype(np.float32), dist=dist)[:, 0]
    assert (want[2] == 0).all() and (want[0, :2, :] != want[1, :2, :]).any() and want[1, H - 1, W - 1] == 0 and (want != drawn).any()
    call = Call(dev, points, table, 4, H, W, off)
    _check(call, want.astype(np.int8), call.run(roi=dist))


# ================================================================================================ rough_ROI
def _roi(dev, data, dist=20, off=0, in_place=False, **over):
    """ivosw_rough_roi on float32 [b,1,h,w] inside guard bands: (rc, out, Bufs)."""
    b, _, h, w = data.shape
    b_in = Buf(dev, data, -3.25, off)
    b_out = b_in if in_place else Buf(dev, np.full(data.size, F32_FILL, np.float32), F32_FILL, off)
    need = L.lib().ivosw_rough_roi_ws_bytes(b)
    b_ws = Buf(dev, np.full(max(need, 16), WS_FILL, np.uint8), WS_FILL)
    a = dict(inp=b_in.ptr(), out=b_out.ptr(), b=b, h=h, w=w, dist=dist, ws=b_ws.ptr(), ws_bytes=need)
    a.update(over)
    rc = L.lib().ivosw_rough_roi(a["inp"], a["out"], a["b"], a["h"], a["w"], a["dist"], a["ws"], a["ws_bytes"], L.stream_ptr(dev))
    return rc, (b_in, b_out, b_ws)


def _same_f32(got, want, why):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    np.testing.assert_array_equal(np.where(both_nan, 0, got).view(np.uint32), np.where(both_nan, 0, want).view(np.uint32), err_msg=why)


@pytest.fixture(scope="module")
def fixtures():
    fx = np.load(GOLDEN)
    return {k[3:]: (fx[k].astype(np.float32), fx["out_" + k[3:]].astype(np.float32)) for k in fx.files if k.startswith("in_")}


def test_fused_roi_raster_then_rough_roi_and_the_recorded_reference_agree(dev, fixtures):
    """Every fixture image as one-point paths (so the raster reproduces it exactly): the fused finalise pass, the raster followed by
    ivosw_rough_roi (out of place, in place, and off the 16-byte grid) and the reference's recorded output are the same bits."""
    empty = np.full((1, 1, 30, 40), -1.0, np.float32)
    cases = dict(fixtures, empty=(empty, sr.rough_roi(empty)))
    assert "s_pixel_br" in cases and (cases["s_pixel_br"][0][0, 0, -1, -1] == 1)      # the scribble on the last row and column
    for name, (inp, want) in sorted(cases.items()):
        _same_f32(sr.rough_roi(inp), want, name)
        b, _, h, w = inp.shape
        m, ys, xs = np.nonzero(inp[:, 0] != -1)
        paths = [([(int(x), int(y))], int(inp[k, 0, y, x])) for k, y, x in zip(m, ys, xs)]
        points, table = _table(paths, [int(k) for k in m])
        fused = Call(dev, points, table, b, h, w)
        assert fused.run(roi=20) == 0, (name, L.lib().ivosw_last_error())
        i8, f32 = fused.outputs()
        _same_f32(f32.reshape(inp.shape), want, name + " fused f32")
        np.testing.assert_array_equal(i8.reshape(inp.shape), want.astype(np.int8), err_msg=name + " fused i8")
        plain = Call(dev, points, table, b, h, w, want=("f32",))
        assert plain.run() == 0
        drawn = plain.outputs()[1].reshape(inp.shape)
        _same_f32(drawn, inp, name + " raster")
        for off, in_place in ((0, False), (0, True), (1, False), (1, True)):
            rc, (b_in, b_out, b_ws) = _roi(dev, drawn, off=off, in_place=in_place)
            assert rc == 0, L.lib().ivosw_last_error()
            b_ws.back("ws")
            if not in_place:
                b_in.back("in", unchanged=True)
            _same_f32(b_out.back("out").reshape(inp.shape), want, f"{name} rough_roi off={off} in_place={in_place}")


def test_scalar_switch_gives_the_vector_kernels_bits(dev, monkeypatch):
    """IVOSW_SCRIBBLE_SCALAR on 16-byte aligned buffers: the finalise pass and the rough_roi fill run element by element and give the
    bytes of the 16- and 4-pixel kernels.  Two maps of 5 x 8 (80 pixels: five whole 16-pixel groups, the third spans both maps)."""
    H, W = 5, 8
    points, table = _table([([(1, 1), (6, 3)], 3), ([(7, 4)], 126), ([(0, 0), (7, 0)], 0)], [0, 1, 1])
    want = sr.rough_roi(sr.raster(points, table, 2, H, W)[:, None].astype(np.float32), dist=1)[:, 0]
    drawn = sr.raster(points, table, 2, H, W)[:, None].astype(np.float32)
    got = {}
    for scalar in (False, True):
        if scalar:
            monkeypatch.setenv("IVOSW_SCRIBBLE_SCALAR", "1")                          # read by the launcher at every call
        call = Call(dev, points, table, 2, H, W)
        _check(call, want.astype(np.int8), call.run(roi=1))
        rc, (b_in, b_out, b_ws) = _roi(dev, drawn, dist=1)
        assert rc == 0, L.lib().ivosw_last_error()
        b_in.back("in", unchanged=True)
        b_ws.back("ws")
        got[scalar] = call.outputs() + (b_out.back("out"),)
    for v, s in zip(got[False], got[True]):
        np.testing.assert_array_equal(v.view(np.uint8), s.view(np.uint8))
    _same_f32(got[True][2].reshape(drawn.shape), sr.rough_roi(drawn, dist=1), "rough_roi under the scalar switch")


def test_rough_roi_nan_counts_other_distances_and_default(dev):
    m = np.full((2, 1, 33, 65), -1.0, np.float32)
    m[0, 0, 3, 4] = np.nan
    m[0, 0, 5, 60] = 2.0
    m[1, 0, 32, 0] = 0.0
    for dist in (0, 1, 20, 1 << 30):
        rc, (b_in, b_out, b_ws) = _roi(dev, m, dist=dist)
        assert rc == 0
        _same_f32(b_out.back("out").reshape(m.shape), sr.rough_roi(m, dist=min(dist, 100)), f"dist {dist}")
    # the fused pass with a default other than -1: every pixel counts, the box is the whole map
    points, table = _table([([(2, 2), (9, 4)], 3)])
    call = Call(dev, points, table, 1, 7, 12)
    drawn = sr.raster(points, table, 1, 7, 12, default_value=4)
    _check(call, sr.rough_roi(drawn[:, None].astype(np.float32))[:, 0].astype(np.int8), call.run(default=4, roi=2))


# ================================================================================================ host functions
def _schema(n_frames, per_frame):
    return dict(sequence="s", scribbles=[[dict(path=[list(p) for p in pts], object_id=o, start_time=0, end_time=0)
                                          for pts, o in per_frame.get(f, [])] for f in range(n_frames)])


@pytest.fixture(scope="module")
def two_frames():
    rng = np.random.default_rng(5)
    robot = lambda: [tuple(p) for p in np.clip(np.cumsum(np.vstack([rng.random((1, 2)), rng.normal(0, 0.02, (59, 2))]), 0), 0.0, 1.0)]
    return _schema(2, {0: [(robot(), 1), (robot(), 2), ([(0.0, 0.0), (1.0, 1.0)], 0), ([(1.0, 0.0)], 3), ([], 2)],
                       1: [(robot(), 3), ([(1.0, 0.25), (0.0, 1.0), (0.999999, 0.999999)], 1)]})


def test_scribbles2mask_scribble_maps_and_scribble_label_equal_the_definition(dev, two_frames):
    from ivos_w_amd.utils import utils_manet
    for H, W in ((30, 53), (120, 214)):
        ref = sr.scribbles2mask(two_frames, (H, W))
        assert ref[0, 0, W - 1] == 3 and ref[0, H - 1, W - 1] == 0                    # coordinates of exactly 1.0: the last pixel
        got = S.scribbles2mask(two_frames, (H, W))
        assert got.dtype == torch.int8 and got.is_cuda and tuple(got.shape) == (2, H, W)
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
        np.testing.assert_array_equal(S.scribbles2mask(two_frames, (H, W), bresenham=False, default_value=0).cpu().numpy(),
                                      sr.scribbles2mask(two_frames, (H, W), bresenham=False, default_value=0))
        np.testing.assert_array_equal(S.scribble_maps(two_frames, (H, W), frames=[1], device=dev).cpu().numpy(), ref[1:])
        np.testing.assert_array_equal(S.scribble_maps(two_frames, (H, W), device=dev, as_float=True).cpu().numpy(), ref.astype(np.float32))
        for frame in (0, 1):
            plain = utils_manet.scribble_label(two_frames, frame, (H, W), False, dev)
            first = utils_manet.scribble_label(two_frames, frame, (H, W), True, dev)
            want = ref[frame][None, None].astype(np.float32)
            assert plain.dtype == torch.float32 and tuple(plain.shape) == (1, 1, H, W) and tuple(first.shape) == (1, 1, H, W)
            _same_f32(plain.cpu().numpy(), want, "scribble_label")
            _same_f32(first.cpu().numpy(), sr.rough_roi(want), "scribble_label, first scribble")
            _same_f32(utils_manet.rough_ROI(plain).cpu().numpy(), sr.rough_roi(want), "rough_ROI")
            _same_f32(plain.cpu().numpy(), want, "rough_ROI wrote its input")
    assert tuple(S.scribble_maps(_schema(3, {}), (4, 5), device=dev).shape) == (0, 4, 5)
    assert (utils_manet.scribble_label(_schema(3, {}), 1, (4, 5), True, dev) == 0).all()          # where the reference raises
    assert (utils_manet.scribble_label(_schema(3, {}), 1, (4, 5), False, dev) == -1).all()


def test_ipn_chain_equals_the_dilation_of_the_reference_map(dev, two_frames):
    from ivos_w_amd.utils import utils_ipn
    for H, W in ((30, 53), (480, 854)):
        ref = sr.scribbles2mask(two_frames, (H, W))
        for frame in (0, 1):
            got = utils_ipn.scribble_input(two_frames, frame, (H, W), 3, device=dev)
            want = utils_ipn.dilate_scribbles(torch.from_numpy(ref[frame]).to(dev), 3)
            assert got.dtype == torch.int8 and tuple(got.shape) == (H, W) and int((got >= 0).sum()) > int((ref[frame] >= 0).sum())
            assert torch.equal(got, want)


# ================================================================================================ refusals
def test_refusals_return_their_code_and_leave_every_buffer_alone(dev):
    lib = L.lib()
    paths = [([(0, 0), (8, 3)], 1), ([(8, 0), (0, 6)], 126)]
    points, table = _table(paths, [0, 1])

    def bad_table(row, col, value):
        t = table.copy()
        t[row, col] = value
        return t.ctypes.data, t

    cases = [(dict(points=None), ERR_ARG, "points"), (dict(paths=None), ERR_ARG, "paths"), (dict(paths_host=None), ERR_ARG, "paths_host"),
             (dict(out_i8=None, out_f32=None), ERR_ARG, "out_i8"), (dict(ws=None), ERR_ARG, "ws"), (dict(n_maps=0), ERR_ARG, "n_maps"),
             (dict(H=0), ERR_ARG, "H"), (dict(W=-3), ERR_ARG, "W"), (dict(n_paths=-1), ERR_ARG, "n_paths"), (dict(n_points=-1), ERR_ARG, "n_points"),
             (dict(default=128), ERR_ARG, "default_value"), (dict(n_maps=1 << 30), ERR_ARG, "above 2^31 - 1 pixels"),
             (dict(ws="off grid"), ERR_ARG, "ws off the 16-byte grid"), (dict(ws_bytes=15), ERR_WS, "workspace")]
    for row, col, value, word in ((1, 2, 127, "object id"), (0, 2, -1, "object id"), (1, 3, 2, "map index"), (0, 3, -1, "map index"),
                                  (1, 1, 3, "point range"), (0, 0, -1, "point range"), (1, 1, 0, "point range"), (1, 0, 1, "previous path")):
        ptr, keep = bad_table(row, col, value)
        cases.append((dict(paths_host=ptr, _keep=keep), ERR_ARG, word))
    for over, code, word in cases:
        over = dict(over)
        over.pop("_keep", None)
        call = Call(dev, points, table, 2, 7, 9)
        if "ws_bytes" in over:
            over["ws_bytes"] = call.need - 1
        if over.get("ws") == "off grid":
            over["ws"] = ctypes.c_void_p(call.b_ws.ptr().value + 8)
        assert call.run(**over) == code, (over, lib.ivosw_last_error())
        assert word.encode() in lib.ivosw_last_error(), (word, lib.ivosw_last_error())
        call.outputs(unchanged=True)
    m = np.full((1, 1, 7, 9), -1.0, np.float32)
    m[0, 0, 2, 2] = 1.0
    for over, code, word in ((dict(inp=None), ERR_ARG, "null in"), (dict(out=None), ERR_ARG, "null out"), (dict(ws=None), ERR_ARG, "null ws"),
                             (dict(b=0), ERR_ARG, "b, h and w must be positive"), (dict(h=0), ERR_ARG, "b, h and w must be positive"),
                             (dict(w=-1), ERR_ARG, "b, h and w must be positive"), (dict(dist=-1), ERR_ARG, "dist < 0"),
                             (dict(b=65536), ERR_ARG, "b above 65535"), (dict(b=3, h=1 << 15, w=1 << 15), ERR_ARG, "b * h * w above 2^31 - 1"),
                             (dict(ws_bytes=15), ERR_WS, "workspace")):
        rc, bufs = _roi(dev, m, **over)
        assert rc == code and word.encode() in lib.ivosw_last_error(), (over, lib.ivosw_last_error())
        for b in bufs:
            b.back("rough_roi buffer", unchanged=True)
    # a call with n_paths = 0 needs none of the three path arguments
    call = Call(dev, [], [], 1, 3, 3)
    _check(call, np.full((1, 3, 3), -1, np.int8), call.run(points=None, paths=None, paths_host=None))


# ================================================================================================ the option
def test_run_eval_with_real_paths(dev, tmp_path, monkeypatch, capsys):
    """scribbles=paths on one tiny sequence: the session hands out real paths, run_eval draws them at the stand-in's stride-4 resolution
    and the stand-in's output carries the scribbled object's label at the scribbled pixels of the annotated frame."""
    from ivos_w_amd import entry
    seen = []
    real = entry.StandInVOS.logits

    def spy(self, gt_u8, n_objects, annotated_frames, scribble_low=None):
        out = real(self, gt_u8, n_objects, annotated_frames, scribble_low=scribble_low)
        seen.append((scribble_low, out.argmax(1), gt_u8, n_objects, list(annotated_frames)))
        return out
    monkeypatch.setattr(entry.StandInVOS, "logits", spy)
    common = ["with", "synthetic=1", "setting=oracle", "method=ours", "synth.n_sequences=1", "synth.n_frames=5", "synth.height=48",
              "synth.width=64", "eval_max_nb_interactions=3", f"ckpt_dir={tmp_path}/weights"]
    out = entry.run_eval(entry.parse_cli(common + ["scribbles=paths", f"report_save_dir={tmp_path}/paths"]), "MANet")
    text = capsys.readouterr().out
    assert len(seen) == 3 and text.count("scribble: ") == 3 and len(out["curve"]["J_AND_F"]) == 3
    for scribble_low, label_low, gt, n_objects, annotated in seen:
        frame, low = scribble_low
        assert frame == annotated[-1] and low.dtype == torch.int8 and tuple(low.shape) == (12, 16) and low.is_cuda
        sc = dict(scribbles=[entry.robot_paths(gt[f].cpu().numpy(), n_objects) if f == frame else [] for f in range(5)])
        assert f"scribble: {len(sc['scribbles'][frame])} paths" in text and len(sc["scribbles"][frame]) >= 1
        want = sr.scribbles2mask(sc, (12, 16))[frame]
        np.testing.assert_array_equal(low.cpu().numpy(), want)
        ys, xs = np.nonzero(want >= 0)
        assert len(ys) >= 1 and (label_low[frame].cpu().numpy()[ys, xs] == want[ys, xs]).all()
    # the default: no path is drawn, the stand-in is called as it was, the log line is what it was
    seen.clear()
    entry.run_eval(entry.parse_cli(common + [f"report_save_dir={tmp_path}/frame"]), "MANet")
    assert len(seen) == 3 and all(s[0] is None for s in seen) and "scribble: " not in capsys.readouterr().out
