"""CPU: the host side of the scribble rasteriser - the closed form of the line rule against its loop, packing, the schema, the numpy
rough_ROI against the recorded reference function, the ``scribbles`` option and the synthetic robot's paths."""
import copy
import os

import numpy as np
import pytest
import torch

from ivos_w_amd import entry
from ivos_w_amd.utils import scribbles as S
from tests import scribble_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scribble_fixtures.npz")


def _schema(n_frames, per_frame):
    """davisinteractive's dict from {frame: [(points, object id), ...]}."""
    return dict(sequence="s", scribbles=[[dict(path=[list(p) for p in pts], object_id=o, start_time=0, end_time=0)
                                          for pts, o in per_frame.get(f, [])] for f in range(n_frames)])


# ------------------------------------------------------------------------------------------------ the line rule
def test_closed_form_equals_the_loop_for_all_lengths_up_to_64():
    for a in range(1, 65):
        for b in range(0, a + 1):
            assert [sr.minor_closed(a, b, s) for s in range(a + 1)] == sr.minor_loop(a, b), (a, b)
    assert sr.minor_loop(0, 0) == [0]


def test_line_loop_octants_and_ties():
    assert sr.line_loop(2, 2, 2, 2) == [(2, 2)]                                       # zero length: one pixel
    assert sr.line_loop(0, 0, 3, 0) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert sr.line_loop(3, 0, 0, 0) == [(3, 0), (2, 0), (1, 0), (0, 0)]
    assert sr.line_loop(0, 3, 0, 0) == [(0, 3), (0, 2), (0, 1), (0, 0)]
    assert sr.line_loop(0, 0, 3, 3) == [(0, 0), (1, 1), (2, 2), (3, 3)]               # dx == dy: y drives
    assert sr.line_loop(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]       # D >= 0 at the first step: the tie goes up
    for x1, y1 in ((5, 2), (2, 5), (-2, 5), (-5, 2), (-5, -2), (-2, -5), (2, -5), (5, -2)):
        pix = sr.line_loop(10, 10, 10 + x1, 10 + y1)
        assert pix[0] == (10, 10) and pix[-1] == (10 + x1, 10 + y1) and len(pix) == 6


# ------------------------------------------------------------------------------------------------ packing and the schema
def test_pack_truncates_and_clamps_one():
    H, W = 7, 5
    sc = _schema(1, {0: [([(0.0, 0.0), (1.0, 1.0), (0.999, 0.5), (0.2, 0.2857142857142857), (0.39999999, 0.6)], 3)]})
    points, table, frames = S.pack(sc, (H, W))
    assert frames == [0] and table.tolist() == [[0, 5, 3, 0]] and points.dtype == np.int32 and table.dtype == np.int32
    assert points.tolist() == [[0, 0], [W - 1, H - 1], [4, 3], [1, int(0.2857142857142857 * 7)], [1, 4]]
    assert points.tolist() == [list(sr.pack_point(x, y, H, W)) for x, y in sc["scribbles"][0][0]["path"]]


@pytest.mark.parametrize("bad", [(-1e-9, 0.5), (0.5, 1.0000001), (float("nan"), 0.5), (0.5, float("inf"))])
def test_pack_refuses_bad_coordinates_naming_frame_and_path(bad):
    sc = _schema(4, {2: [([(0.1, 0.1)], 1), ([(0.5, 0.5), bad], 2)]})
    with pytest.raises(ValueError, match=r"frame 2, path 1"):
        S.pack(sc, (10, 10))


def test_pack_refuses_bad_objects_frames_and_shapes():
    with pytest.raises(ValueError, match="object_id 127"):
        S.pack(_schema(1, {0: [([(0.1, 0.1)], 127)]}), (4, 4))
    with pytest.raises(ValueError, match="object_id -1"):
        S.pack(_schema(1, {0: [([(0.1, 0.1)], -1)]}), (4, 4))
    sc = _schema(3, {1: [([(0.1, 0.1)], 1)]})
    for frames in ([3], [-1], [1, 1]):
        with pytest.raises(ValueError, match="frames"):
            S.pack(sc, (4, 4), frames)
    with pytest.raises(ValueError, match="positive"):
        S.pack(sc, (0, 4))
    with pytest.raises(ValueError, match=r"frame 1, path 0"):
        S.pack(dict(scribbles=[[], [dict(frame=1)], []]), (4, 4), [1])
    with pytest.raises(NotImplementedError, match="bezier"):
        S.scribbles2mask(sc, (4, 4), bezier_curve=True)


def test_pack_frame_list_empty_frames_and_empty_paths():
    sc = _schema(6, {1: [([(0.5, 0.5)], 1), ([], 2), ([(0.1, 0.1), (0.9, 0.9)], 0)], 4: [([], 1)], 5: [([(0.3, 0.3)], 126)]})
    points, table, frames = S.pack(sc, (10, 20))
    assert frames == [1, 5]                                                           # frame 4 has only an empty path
    assert table.tolist() == [[0, 1, 1, 0], [1, 2, 0, 0], [3, 1, 126, 1]] and len(points) == 4
    points, table, frames = S.pack(sc, (10, 20), [5, 0, 1])                            # the caller's order is the map order
    assert frames == [5, 0, 1] and table.tolist() == [[0, 1, 126, 0], [1, 1, 1, 2], [2, 2, 0, 2]]
    points, table, frames = S.pack(_schema(3, {}), (10, 20))
    assert frames == [] and points.shape == (0, 2) and table.shape == (0, 4)
    points, table, frames = S.pack(_schema(3, {}), (10, 20), [2])
    assert frames == [2] and table.shape == (0, 4)
    # the packed form and the schema give the same reference maps
    full = sr.scribbles2mask(sc, (10, 20))
    points, table, frames = S.pack(sc, (10, 20), range(6))
    np.testing.assert_array_equal(sr.raster(points, table, 6, 10, 20), full)
    assert (full[4] == -1).all() and full[1, 5, 10] == 0 and full[1, 1, 2] == 0 and full[5, 3, 6] == 126          # (10, 5): the later path wins


def test_device_entries_have_no_cpu_fallback():
    from ivos_w_amd.utils import utils_manet
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.scribble_maps(_schema(1, {0: [([(0.5, 0.5)], 1)]}), (4, 4), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils_manet.rough_ROI(torch.zeros(1, 1, 4, 4))


# ------------------------------------------------------------------------------------------------ rough_ROI
def test_ref_rough_roi_equals_the_recorded_reference():
    fx = np.load(GOLDEN)
    names = sorted(k[3:] for k in fx.files if k.startswith("in_"))
    assert len(names) >= 20 and {"s_pixel_br", "s_touch_bottom", "l_far", "l_near", "s_batch2", "l_batch2"} <= set(names)
    for name in names:
        m = fx["in_" + name].astype(np.float32)
        np.testing.assert_array_equal(sr.rough_roi(m), fx["out_" + name].astype(np.float32), err_msg=name)
    # the exclusive ends: a scribble on the last row and column loses them, the whole image keeps all but them
    br = fx["out_s_pixel_br"]
    assert br[0, 0, -1, -1] == 0 and (br[0, 0, 9:29, 19:39] == -1).all() and (br == 0).sum() == 30 * 40 - 20 * 20          # the scribble itself is gone
    full = fx["out_s_touch_all"]
    assert (full[0, 0, -1] == 0).all() and (full[0, 0, :, -1] == 0).all() and (full[0, 0, :-1, :-1] == fx["in_s_touch_all"][0, 0, :-1, :-1]).all()
    # the one stated difference: an empty image is all 0 here, and a NaN counts as a pixel
    assert (sr.rough_roi(np.full((1, 1, 5, 6), -1.0, np.float32)) == 0).all()
    m = np.full((1, 1, 30, 40), -1.0, np.float32)
    m[0, 0, 3, 4] = np.nan
    got = sr.rough_roi(m)
    assert np.isnan(got[0, 0, 3, 4]) and got[0, 0, 22, 23] == -1 and got[0, 0, 23, 23] == 0 and got[0, 0, 22, 24] == 0


# ------------------------------------------------------------------------------------------------ the option
def _cfg(**kw):
    return entry.parse_cli([f"{k}={v}" for k, v in kw.items()])


def test_scribbles_option_and_default():
    assert entry.DEFAULTS["scribbles"] == "frame" and entry.SCRIBBLE_MODES == ("frame", "paths")
    assert entry.scribbles_option(_cfg()) == "frame" and entry.scribbles_option({}) == "frame"
    assert entry.scribbles_option(_cfg(scribbles="paths")) == "paths"
    for bad in ("lines", 1, None, True):
        with pytest.raises(ValueError, match="scribbles must be 'frame' or 'paths'"):
            entry.scribbles_option(dict(scribbles=bad))
    with pytest.raises(SystemExit, match="scribbles must be"):
        _cfg(scribbles="curves")


@pytest.fixture(scope="module")
def davis():
    cfg = _cfg(seed=3)
    cfg.synth.n_sequences, cfg.synth.n_frames, cfg.synth.height, cfg.synth.width = 2, 6, 48, 64
    cfg.data.subset = "val"
    return entry.SyntheticDavis(cfg, torch.device("cpu"))


def test_default_session_scribbles_are_what_they_were(davis):
    sess = entry.SyntheticSession(davis, "val", "J_AND_F", 2, "unused", seed=3)
    assert sess.next()
    seq, sc, first = sess.get_scribbles(only_last=True)
    f = sc["annotated_frame"]
    assert first and sc == dict(sequence=seq, annotated_frame=f, scribbles=[[dict(frame=f)] if k == f else [] for k in range(6)])


def test_robot_paths_lie_on_their_objects_and_round_trip(davis):
    sess = entry.SyntheticSession(davis, "val", "J_AND_F", 2, "unused", seed=3, scribbles="paths")
    seen = 0
    while sess.next():
        seq, sc, _ = sess.get_scribbles(only_last=True)
        f = sc["annotated_frame"]
        gt = davis.load_annotations(seq)[f].numpy()
        H, W = gt.shape
        assert [len(p) for k, p in enumerate(sc["scribbles"]) if k != f] == [0] * 5
        paths = sc["scribbles"][f]
        assert [p["object_id"] for p in paths] == [o for o in range(1, davis.dataset[seq]["num_objects"] + 1) if (gt == o).any()]
        points, table, frames = S.pack(sc, (H, W))
        assert frames == [f] and len(table) == len(paths)
        for (first, n, obj, m), p in zip(table.tolist(), paths):
            assert sorted(p) == ["end_time", "object_id", "path", "start_time"] and 1 <= n <= 5 and m == 0
            px = points[first:first + n]
            assert (gt[px[:, 1], px[:, 0]] == obj).all()                              # the points are pixels of the object ...
            assert [[(x + 0.5) / W, (y + 0.5) / H] for x, y in px.tolist()] == p["path"]          # ... and round-trip exactly
        full = sr.raster(points, table, 1, H, W)[0]                                   # every pixel the polylines cross is the object's
        assert (full[full >= 0] == gt[full >= 0]).all() and (full >= 0).sum() >= len(paths)
        assert entry.robot_paths(gt, davis.dataset[seq]["num_objects"]) == paths      # deterministic
        seen += 1
    assert seen == 2


def test_stand_in_takes_the_scribbled_label_and_is_unchanged_without(davis):
    seq = davis.sets["val"][0]
    gt, n_obj = davis.load_annotations(seq), davis.dataset[seq]["num_objects"]
    vos = entry.StandInVOS(torch.device("cpu"), seed=3)
    base = vos.logits(gt, n_obj, [2])
    sc = dict(scribbles=[entry.robot_paths(gt[2].numpy(), n_obj) if f == 2 else [] for f in range(6)])
    low = sr.scribbles2mask(sc, (12, 16))[2]
    got = vos.logits(gt, n_obj, [2], scribble_low=(2, torch.from_numpy(low)))
    assert torch.equal(vos.logits(gt, n_obj, [2]), base)
    ys, xs = np.nonzero(low >= 0)
    assert len(ys) > 0
    want = base.clone()
    want[2, torch.from_numpy(low[ys, xs].astype(np.int64)), torch.from_numpy(ys), torch.from_numpy(xs)] += 8.0
    assert torch.equal(got, want)
    assert (got[2].argmax(0).numpy()[ys, xs] == low[ys, xs]).all()
