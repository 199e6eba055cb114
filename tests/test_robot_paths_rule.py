"""CPU: the level-synchronous statement of the robot's path step (tests/robot_paths_ref.py, the rule of ``ivosw_robot_paths``) gives
what the FIFO statement of tests/robot_ref.py gives - on hand-made shapes, on random skeletons, and for the resampling expression."""
import numpy as np

from tests import robot_paths_ref as P
from tests import robot_ref as R


def test_hand_made_shapes_match_the_fifo_statement():
    shapes, _ = P.hand_shapes()
    assert len(shapes) >= 14
    for name, pixels, kw in shapes:
        a = dict(min_nb_nodes=4, max_paths=2)
        a.update(kw)
        assert P.longest_paths(pixels, **a) == R.longest_paths(pixels, **a), name
    ring = dict((n, p) for n, p, _ in shapes)["ring"]
    assert len(R.longest_paths(ring, 4, 2)[0]) == 5                # two equal routes round the ring: the parent rule picked one
    joined = dict((n, p) for n, p, _ in shapes)["row end and next row start"]
    assert [len(p) for p in R.longest_paths(joined, 4, 2)] == [4, 4]


def test_random_skeletons_match_the_fifo_statement():
    seen = 0
    for seed in range(200):
        sk, _ = R.thin_fast(R.blob(40, 70, seed))
        pixels = [(int(y), int(x)) for y, x in zip(*np.nonzero(sk))]
        for min_nb, max_paths in ((4, 2), (1, 8)):
            want = R.longest_paths(pixels, min_nb, max_paths)
            assert P.longest_paths(pixels, min_nb, max_paths) == want, (seed, min_nb, max_paths)
            seen += len(want)
    assert seen > 400


def test_resampling_expression_is_linspace_round_unique():
    for length in range(1, 301):
        path = list(range(length))
        for nb in range(1, 17):
            assert P.resample_indices(length, nb) == R.resample(path, nb), (length, nb)


def test_device_paths_layout_of_the_restatement():
    shapes, _ = P.hand_shapes()
    pix = dict((n, p) for n, p, _ in shapes)["three components, max_paths 2"]
    pts = np.stack([P.points_of_pixels(pix, 32), P.points_of_pixels(pix, 32), P.points_of_pixels([], 32)])
    nodes, lens, status = P.device_paths(pts, np.array([len(pix), 33, 0]), 4, 2, None, 5)
    assert status.tolist() == [2, 1, 0] and lens.tolist() == [[0, 5], [0, 0], [0, 0]]
    assert (nodes[0, 0] == -1).all() and (nodes[1] == -1).all() and (nodes[2] == -1).all()
    assert nodes[0, 1].tolist() == [[x, 7] for x in range(5, 0, -1)]       # a -> b: a is the node farthest from the first pixel
    nodes, lens, status = P.device_paths(pts[:1], np.array([len(pix)]), 4, 2, 3, 4)
    assert status.tolist() == [0] and lens.tolist() == [[3, 3]]
    assert nodes[0, 0].tolist() == [[6, 4], [4, 4], [1, 4], [1, 4]] and nodes[0, 1].tolist() == [[5, 7], [3, 7], [1, 7], [1, 7]]
