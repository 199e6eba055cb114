"""CPU: the host side of the error-driven scribble robot - the per-pixel restatement of the thinning rule (tests/robot_ref.py) on
hand-written skeletons, its agreement with the tabulated form, the path step of utils/robot.py (components, double BFS, ties, resampling)
and the ``robot`` option."""
import numpy as np
import pytest
from scipy import ndimage

from ivos_w_amd import entry
from ivos_w_amd.utils import robot as R
from tests import robot_ref as rr

EIGHT, blob = rr.EIGHT, rr.blob


def _plane(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def _text(plane):
    return ["".join("#" if v else "." for v in r) for r in plane]


# ------------------------------------------------------------------------------------------------ the thinning rule
HAND = {
    # a 3 x 7 bar.  Sub-iteration 1 takes the south row, the east column's middle pixel and all four corners (the north row has
    # P4 * P6 * P8 = 1, the west pixel P2 * P4 * P6 = 1).  Sub-iteration 2 takes what is left of the north row (P2 = 0), the west pixel
    # (1, 0) (B = 2: NE and E) and (1, 5) (B = 3: N, W, NW; P4 = P6 = 0); (1, 1) has A = 2, (1, 2 .. 4) have P2 * P4 * P8 = 1.  The row of
    # four that is left has end points (B = 1) and line pixels (A = 2): the second iteration deletes nothing.
    "bar": (["#######", "#######", "#######"], [".......", ".####..", "......."], 1),
    # a plus with arms of one pixel above and below a row of five: the two arm pixels see SE, S, SW (or NW, N, NE): B = 3, A = 1 and a
    # clear P2 or P6, so both go in sub-iteration 1; the row's pixels next to the centre have A = 2, its ends B = 1
    "plus": ([".....", "..#..", "#####", "..#..", "....."], [".....", ".....", "#####", ".....", "....."], 1),
    # an L of one-pixel strokes is a skeleton already: the corner has N and E set (B = 2, but A = 2), the strokes A = 2, the ends B = 1
    "L": (["#...", "#...", "#...", "####"], ["#...", "#...", "#...", "####"], 0),
    # the algorithm's known artefact: every pixel of an isolated 2 x 2 block has B = 3 and A = 1; sub-iteration 1 takes (1, 1) (P4 = P6 = 0
    # fails nothing), ... and the block is deleted whole within one iteration
    "block": (["....", ".##.", ".##.", "...."], ["....", "....", "....", "...."], 1),
    "pixel": (["...", ".#.", "..."], ["...", ".#.", "..."], 0),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_written_skeletons(name):
    rows, want, iters = HAND[name]
    sk, it = rr.thin(_plane(rows))
    assert _text(sk) == want and it == iters
    sk2, it2 = rr.thin_fast(_plane(rows))
    assert _text(sk2) == want and it2 == iters


def test_rule_on_single_neighbourhoods():
    # P2 .. P9 = N, NE, E, SE, S, SW, W, NW
    assert rr.deletable((1, 1, 1, 0, 0, 0, 0, 0), 0) and rr.deletable((1, 1, 1, 0, 0, 0, 0, 0), 1)          # a convex corner: B = 3, A = 1
    assert not rr.deletable((1, 0, 0, 0, 0, 0, 0, 0), 0)                                                    # an end point: B = 1
    assert not rr.deletable((1, 0, 0, 0, 1, 0, 0, 0), 0)                                                    # a line: A = 2
    assert not rr.deletable((1, 1, 1, 1, 1, 1, 1, 0), 0)                                                    # B = 7
    south_side = (1, 1, 1, 0, 0, 0, 1, 1)                                                                   # N, E, W set, S clear: B = 5, A = 1
    assert rr.deletable(south_side, 0) and not rr.deletable(south_side, 1)                                  # P2 * P4 * P8 = 1 bars sub-iteration 2
    north_side = (0, 0, 1, 1, 1, 1, 1, 0)
    assert rr.deletable(north_side, 1) and not rr.deletable(north_side, 0)                                  # P4 * P6 * P8 = 1 bars sub-iteration 1
    assert int(rr._table().sum()) == sum(rr.deletable([(c >> k) & 1 for k in range(8)], s) for c in range(256) for s in (0, 1))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pixelwise_and_tabulated_forms_agree_and_keep_the_topology(seed):
    for H, W in ((17, 33), (31, 65), (3, 96)):
        plane = blob(H, W, seed)
        assert plane.any() and not plane.all()
        sk, it = rr.thin(plane)
        sk2, it2 = rr.thin_fast(plane)
        assert (sk == sk2).all() and it == it2 and it >= 0
        assert not (sk & ~plane).any()
        lab, n = ndimage.label(plane, EIGHT)
        sizes = ndimage.sum(plane, lab, range(1, n + 1))
        boxes = ndimage.find_objects(lab)
        two_by_two = sum(1 for k in range(n) if sizes[k] == 4 and all(s.stop - s.start == 2 for s in boxes[k]))
        assert ndimage.label(sk, EIGHT)[1] == n - two_by_two


def test_bit_plane_and_point_forms():
    plane = blob(5, 70, 3)
    words = rr.pack_bits(plane)
    assert words.shape == (5, 3) and words.dtype == np.uint32 and (rr.unpack_bits(words, 70) == plane).all()
    assert (words[:, 2] >> 6 == 0).all()                                                                    # bits at x >= W are 0
    pts = rr.points_of(plane)
    assert [(int(p) >> 16, int(p) & 0xffff) for p in pts] == sorted(zip(*(a.tolist() for a in np.nonzero(plane))))
    gt = np.array([[1, 1, 2], [1, 0, 2]], np.uint8)
    pred = np.array([[1, 0, 2], [2, 1, 1]], np.uint8)
    assert rr.error_plane(gt, pred, 1).tolist() == [[False, True, False], [True, False, False]]
    assert rr.error_plane(gt, None, 2).tolist() == [[False, False, True], [False, False, True]]


# ------------------------------------------------------------------------------------------------ the path step
def _points(pixels, cap=None):
    pts = np.array([(y << 16) | x for y, x in sorted(pixels)], np.int32)
    return pts if cap is None else np.concatenate([pts, np.full(cap - len(pts), -1, np.int32)])


def _adjacent(path):
    return all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(path, path[1:]))


def test_paths_follow_the_skeleton():
    for seed in (0, 1, 2):
        sk, _ = rr.thin_fast(blob(40, 60, seed))
        pixels = sorted(zip(*(a.tolist() for a in np.nonzero(sk))))
        paths = R.longest_paths(pixels, min_nb_nodes=1, max_paths=100)
        assert paths == rr.longest_paths(pixels, 1, 100) and len(paths) == ndimage.label(sk, EIGHT)[1]
        for p in paths:
            assert _adjacent(p) and set(p) <= set(pixels) and len(set(p)) == len(p)
        assert [len(p) for p in paths] == sorted((len(p) for p in paths), reverse=True)
        assert R.longest_paths(pixels) == paths[:2] if len(paths[1]) >= 4 else True


def test_double_bfs_finds_the_diameter_of_a_tree():
    # a T: the stem hangs from the middle of the bar; the longest shortest path joins the two far ends
    bar = [(2, x) for x in range(1, 12)]
    stem = [(y, 6) for y in range(3, 7)]
    (path,) = R.longest_paths(sorted(bar + stem))
    assert _adjacent(path) and len(path) == 11
    assert path[0] == (2, 11) and path[-1] == (2, 1)      # the first BFS starts at the first pixel (2, 1) and finds a = (2, 11); the path runs a -> b
    # a longer stem: from (2, 1) the foot (11, 6) is the farthest (13 steps; the diagonal step (2, 5) -> (3, 6) saves one), from there both
    # ends of the bar are 13 steps away and the lower raster index (2, 1) wins
    stem = [(y, 6) for y in range(3, 12)]
    (path,) = R.longest_paths(sorted(bar + stem))
    assert _adjacent(path) and len(path) == 14 and path[0] == (11, 6) and path[-1] == (2, 1)


def test_min_nb_nodes_max_paths_and_ties():
    three = [(0, x) for x in range(3)]
    four = [(4, x) for x in range(10, 14)]
    six_a = [(8, x) for x in range(6)]
    six_b = [(8, x) for x in range(20, 26)]
    nine = [(y, 30) for y in range(12, 21)]
    pixels = sorted(three + four + six_a + six_b + nine)
    nine, six_a, six_b, four, three = (p[::-1] for p in (nine, six_a, six_b, four, three))        # a line runs from its far end back to its first pixel
    assert R.longest_paths(pixels, min_nb_nodes=4, max_paths=9) == [nine, six_a, six_b, four]       # ties: the lower first pixel first
    assert R.longest_paths(pixels, min_nb_nodes=4, max_paths=2) == [nine, six_a]
    assert R.longest_paths(pixels, min_nb_nodes=5, max_paths=9) == [nine, six_a, six_b]
    assert R.longest_paths(pixels, min_nb_nodes=1, max_paths=9)[-1] == three
    assert R.longest_paths(pixels, min_nb_nodes=10) == [] and R.longest_paths([]) == []
    # a tie between farthest nodes goes to the lower raster index: a closed ring of 8 around (5, 5), from its first pixel (4, 4) the
    # farthest nodes are (6, 5) and (6, 6) (4 steps each) ... whichever the rule picks, both forms pick the same
    ring = sorted((y, x) for y in (4, 5, 6) for x in (4, 5, 6) if (y, x) != (5, 5))
    assert R.longest_paths(ring) == rr.longest_paths(ring)
    # a diagonal: raster order and the neighbour order do not matter, the path is the diagonal from its first pixel
    diag = [(k, 9 - k) for k in range(7)]
    assert R.longest_paths(sorted(diag)) == [sorted(diag)[::-1]]


def test_farthest_tie_goes_to_the_lower_raster_index():
    # a bar with a two-pixel stem standing on its middle: from the first pixel (0, 6) both ends of the bar are 6 steps away (two down the stem
    # with a diagonal step onto the bar, four along it); the lower raster index (2, 1) becomes a, and the path runs from it to (2, 11)
    shape = sorted([(2, x) for x in range(1, 12)] + [(0, 6), (1, 6)])
    (path,) = R.longest_paths(shape)
    assert path[0] == (2, 1) and path[-1] == (2, 11) and len(path) == 11 and _adjacent(path)
    # two shortest paths join them; the neighbour order decides: (2, 5) finds its NE neighbour (1, 6) before its E neighbour (2, 6), and
    # (1, 6), first in the queue, is the one that finds (2, 7)
    assert path[5] == (1, 6)
    assert rr.longest_paths(shape) == [path]


def test_paths_from_points_schema_resampling_and_overflow():
    H, W = 30, 50
    line = [(7, x) for x in range(3, 40)]
    short = [(20, x) for x in range(5)]
    pts = _points(line + short, cap=64)
    got = R.paths_from_points(pts, len(line) + len(short), (H, W), 3)
    assert got == rr.paths_from_points(pts, len(line) + len(short), (H, W), 3) and len(got) == 2
    assert all(sorted(p) == ["end_time", "object_id", "path", "start_time"] and p["object_id"] == 3 for p in got)
    xs = 39 - np.unique(np.linspace(0, 36, 8).round().astype(int))                                         # the path runs from the far end back
    assert got[0]["path"] == [[(int(x) + 0.5) / W, 7.5 / H] for x in xs] and len(got[1]["path"]) == 5
    assert len(R.paths_from_points(pts, len(pts[pts >= 0]), (H, W), 3, nb_points=2)[0]["path"]) == 2
    dense = R.paths_from_points(pts, 42, (H, W), 3, nb_points=None)
    assert [len(p["path"]) for p in dense] == [37, 5]
    assert [[int(x * W), int(y * H)] for x, y in dense[0]["path"]] == [[x, y] for y, x in line[::-1]]    # the points map back to their pixels
    assert R.paths_from_points(pts, 42, (H, W), 3, max_paths=1) == got[:1]
    assert R.paths_from_points(pts, 42, (H, W), 3, min_nb_nodes=6) == got[:1]
    assert R.paths_from_points(pts, 0, (H, W), 3) == []
    with pytest.raises(ValueError, match=r"object 3.*65 pixels.*64"):
        R.paths_from_points(pts, 65, (H, W), 3)


def test_device_entries_have_no_cpu_fallback():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.skeleton_points(torch.zeros(1, 4, 4, dtype=torch.uint8), None, [(0, 1)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.interact(torch.zeros(1, 4, 4, dtype=torch.uint8), None, 1, 0)


# ------------------------------------------------------------------------------------------------ the option
def _cfg(**kw):
    return entry.parse_cli([f"{k}={v}" for k, v in kw.items()])


def test_robot_option_defaults_and_refusals():
    assert entry.DEFAULTS["robot"] == "gt" and entry.DEFAULTS["robot_min_nodes"] == 4 and entry.ROBOT_MODES == ("gt", "errors")
    assert entry.DEFAULTS["scribbles"] == "frame" and entry.SCRIBBLE_MODES == ("frame", "paths")
    assert entry.robot_option(_cfg()) == ("gt", 4) and entry.robot_option({}) == ("gt", 4)
    assert entry.robot_option(_cfg(scribbles="paths", robot="errors", robot_min_nodes=7)) == ("errors", 7)
    assert entry.robot_option(_cfg(scribbles="paths")) == ("gt", 4) and entry.robot_option(_cfg(robot="gt")) == ("gt", 4)
    for bad in ("skeleton", 1, None, True):
        with pytest.raises(ValueError, match="robot must be 'gt' or 'errors'"):
            entry.robot_option(dict(robot=bad, scribbles="paths"))
    for bad in (0, -1, 2.5, "4", True, None):
        with pytest.raises(ValueError, match="robot_min_nodes must be an integer >= 1"):
            entry.robot_option(dict(robot="errors", scribbles="paths", robot_min_nodes=bad))
    with pytest.raises(ValueError, match="needs scribbles=paths"):
        entry.robot_option(dict(robot="errors"))
    with pytest.raises(ValueError, match="needs scribbles=paths"):
        entry.robot_option(dict(robot="errors", scribbles="frame"))
    with pytest.raises(SystemExit, match="robot must be"):
        _cfg(robot="bones")
    with pytest.raises(SystemExit, match="needs scribbles=paths"):
        _cfg(robot="errors")


def test_default_session_never_asks_the_error_robot(monkeypatch):
    import torch
    cfg = _cfg(seed=3)
    cfg.synth.n_sequences, cfg.synth.n_frames, cfg.synth.height, cfg.synth.width = 1, 4, 48, 64
    cfg.data.subset = "val"
    davis = entry.SyntheticDavis(cfg, torch.device("cpu"))
    monkeypatch.setattr(R, "interact", lambda *a, **k: pytest.fail("robot=gt called the error robot"))
    sess = entry.SyntheticSession(davis, "val", "J_AND_F", 2, "unused", seed=3, scribbles="paths")
    assert sess.next() and sess.robot == "gt"
    seq, sc, _ = sess.get_scribbles(only_last=True)
    f = sc["annotated_frame"]
    assert sc["scribbles"][f] == entry.robot_paths(davis.load_annotations(seq)[f].numpy(), davis.dataset[seq]["num_objects"])
    assert sess.drew == "gt" and sess._submitted is None


def test_kernel_has_no_static_lds_no_scratch_and_the_size_query_counts_what_it_uses():
    """The size limit counts two planes and 256 carved bytes, so the code object must bring no LDS of its own (a workgroup reduction
    builtin would: 256 bytes, and the largest accepted size would ask for more than a workgroup may have); no scratch, no spills."""
    import importlib.util
    import os
    from ivos_w_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    lib = L.lib()
    assert lib.ivosw_robot_skeleton_fits(480, 854) == 1 and lib.ivosw_robot_skeleton_fits(720, 1280) == 0
    assert lib.ivosw_robot_skeleton_fits(10224, 40) == 1 and lib.ivosw_robot_skeleton_fits(10225, 40) == 0          # 2 * 10224 * 2 * 4 + 256 = 163840
    assert lib.ivosw_robot_skeleton_fits(0, 1) == 0 and lib.ivosw_robot_skeleton_fits(1, 65536) == 0 and lib.ivosw_robot_skeleton_fits(1, 65535) == 1
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    rows = [r for n, r in kr.kernel_table(L.LIB_PATH).items() if "robot_skeleton_kernel" in n]
    assert len(rows) == 1 and rows[0]["lds"] == 0 and rows[0]["scratch"] == 0 and rows[0]["spill"] == 0 and rows[0]["vgpr"] <= 128, rows
