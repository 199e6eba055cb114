"""GPU: the robot's path step on the device (csrc/robot_paths.hip) through the C ABI and through utils/robot.py against the
level-synchronous restatement of tests/robot_paths_ref.py (which tests/test_robot_paths_rule.py holds to tests/robot_ref.py): nodes, lens
and status bit for bit, padding and (-1, -1) fills included.  Every buffer lies inside a guard band whose fill must survive; a refused
call leaves every buffer as it was."""
import ctypes

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import robot as R
from ivos_w_amd.utils import scribbles as S
from tests import robot_paths_ref as P
from tests import robot_ref as rr

pytestmark = pytest.mark.gpu

PAD, FILL, ERR_ARG = 16, -7, -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class Buf:
    """A device int32 buffer holding ``data`` (flat) PAD elements inside an allocation filled with FILL; ``back()`` returns the data as it
    is now after checking the guard bands."""

    def __init__(self, dev, data):
        data = np.ascontiguousarray(data, np.int32).reshape(-1)
        self.n = data.size
        self.host = np.full(data.size + 2 * PAD, FILL, np.int32)
        self.host[PAD:PAD + self.n] = data
        self.t = torch.from_numpy(self.host).to(dev)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + PAD * 4)

    def back(self, name, unchanged=False):
        h = self.t.cpu().numpy()
        assert (h[:PAD] == FILL).all() and (h[PAD + self.n:] == FILL).all(), f"{name}: written outside its extent"
        if unchanged:
            np.testing.assert_array_equal(h, self.host, err_msg=f"{name}: written by a refused call / an input")
        return h[PAD:PAD + self.n]


def run(dev, points, counts, size, min_nb_nodes=4, max_paths=2, nb_points=None, slot=None, over=None):
    """One ivosw_robot_paths call on host ``points`` int32 [m,cap] and ``counts`` [m] with every buffer in guard bands:
    (rc, message, nodes, lens, status)."""
    points, counts = np.asarray(points, np.int32), np.asarray(counts, np.int32)
    m, cap = points.shape
    slot = cap if slot is None else slot
    nb = 0 if nb_points is None else nb_points
    b = dict(points=Buf(dev, points), counts=Buf(dev, counts), nodes=Buf(dev, np.full(m * max_paths * max(slot, 1) * 2, FILL)),
             lens=Buf(dev, np.full(m * max_paths, FILL)), status=Buf(dev, np.full(m, FILL)))
    a = dict(points=b["points"].ptr(), counts=b["counts"].ptr(), m=m, cap=cap, H=size[0], W=size[1], min_nb_nodes=min_nb_nodes,
             max_paths=max_paths, nb_points=nb, slot=slot, nodes=b["nodes"].ptr(), lens=b["lens"].ptr(), status=b["status"].ptr())
    a.update(over or {})                                           # single C arguments replaced (the buffers keep their sizes)
    rc = L.lib().ivosw_robot_paths(a["points"], a["counts"], a["m"], a["cap"], a["H"], a["W"], a["min_nb_nodes"], a["max_paths"], a["nb_points"],
                                   a["slot"], a["nodes"], a["lens"], a["status"], L.stream_ptr(dev))
    msg = L.lib().ivosw_last_error().decode()
    torch.cuda.synchronize(dev)
    refused = rc != 0
    b["points"].back("points", unchanged=True)
    b["counts"].back("counts", unchanged=True)
    nodes = b["nodes"].back("nodes", unchanged=refused).reshape(m, max_paths, max(slot, 1), 2)
    lens = b["lens"].back("lens", unchanged=refused).reshape(m, max_paths)
    status = b["status"].back("status", unchanged=refused)
    return rc, msg, nodes, lens, status


def check(dev, points, counts, size, **kw):
    rc, msg, nodes, lens, status = run(dev, points, counts, size, **kw)
    assert rc == 0, msg
    want = P.device_paths(points, counts, kw.get("min_nb_nodes", 4), kw.get("max_paths", 2), kw.get("nb_points"),
                          kw.get("slot") or np.asarray(points).shape[1])
    for name, got, ref in zip(("nodes", "lens", "status"), (nodes, lens, status), want):
        np.testing.assert_array_equal(got, ref, err_msg=name)
    return nodes, lens, status


def test_hand_made_shapes_in_one_launch(dev):
    """One unit per shape; units that share (min_nb_nodes, max_paths) share a launch - the default pair is ONE launch of all shapes."""
    shapes, size = P.hand_shapes()
    cap = 64
    for key in sorted({tuple(sorted(kw.items())) for _, _, kw in shapes}):
        mine = [(n, p) for n, p, kw in shapes if tuple(sorted(kw.items())) == key]
        points = np.stack([P.points_of_pixels(p, cap) for _, p in mine])
        counts = [len(p) for _, p in mine]
        for nb in (None, 3):
            nodes, lens, status = check(dev, points, counts, size, nb_points=nb, **dict(key))
            assert (status == 0).all()
        if not key:
            assert len(mine) >= 14
            by = {n: lens[i].tolist() for i, (n, _) in enumerate(mine)}
            assert by["empty"] == [0, 0] and by["one pixel"] == [0, 0] and by["chain of min_nb_nodes - 1"] == [0, 0]
            assert by["chain of min_nb_nodes"] == [3, 0] and by["row end and next row start"] == [3, 3]      # (resampled to 3)
            assert by["diagonal through y = 32768"] == [3, 0]


@pytest.fixture(scope="module")
def skeletons():
    """65 random skeletons at 40 x 70 as (points [65,cap], counts)."""
    cap, pts, counts = 700, [], []
    for seed in range(65):
        p = rr.points_of(rr.thin_fast(rr.blob(40, 70, 1000 + seed))[0])
        assert 0 < len(p) <= cap
        pts.append(np.concatenate([p, np.full(cap - len(p), -1, np.int32)]))
        counts.append(len(p))
    return np.stack(pts), np.array(counts, np.int32)


@pytest.mark.parametrize("nb_points", [None, 1, 8])
@pytest.mark.parametrize("max_paths", [1, 2, 8])
def test_random_skeletons(dev, skeletons, nb_points, max_paths):
    points, counts = skeletons
    nodes, lens, _ = check(dev, points[:64], counts[:64], (40, 70), nb_points=nb_points, max_paths=max_paths, slot=None if nb_points is None else 8)
    assert (lens[:, 0] > 0).sum() > 32


def test_65_units_are_two_groups_and_units_are_independent(dev, skeletons):
    points, counts = skeletons
    nodes, lens, status = check(dev, points, counts, (40, 70), nb_points=8, slot=8)
    again = check(dev, points, counts, (40, 70), nb_points=8, slot=8)
    for a, b in zip((nodes, lens, status), again):                 # determinism: the same launch twice, the same bits
        np.testing.assert_array_equal(a, b)
    for k in (0, 17, 64):                                          # a unit alone and beside the others
        alone = check(dev, points[k:k + 1], counts[k:k + 1], (40, 70), nb_points=8, slot=8)
        np.testing.assert_array_equal(alone[0][0], nodes[k])
        np.testing.assert_array_equal(alone[1][0], lens[k])


def serpentine(n, W=64):
    """A chain of exactly n pixels in which every pixel has at most two neighbours: every other row holds x = 1 .. W - 2, walked to and
    fro, and a single pixel diagonally outside the row end (x = W - 1, then x = 0) joins it to the next one."""
    pix, y, right = [], 0, True
    while len(pix) < n:
        xs = range(1, W - 1)
        pix += [(y, x) for x in (xs if right else reversed(xs))]
        pix.append((y + 1, W - 1 if right else 0))
        y, right = y + 2, not right
    return sorted(pix[:n])


def test_a_chain_that_fills_the_cap_and_one_beyond_it(dev):
    cap = 4096
    assert L.lib().ivosw_robot_paths_max_cap() >= cap
    pix = serpentine(cap)
    points = np.stack([P.points_of_pixels(pix, cap)] * 2)
    nodes, lens, status = check(dev, points, [cap, cap + 1], (200, 64))
    assert status.tolist() == [0, 1] and lens.tolist() == [[cap, 0], [0, 0]] and (nodes[1] == -1).all()
    assert sorted(map(tuple, nodes[0, 0][:, ::-1].tolist())) == pix           # the path is the chain
    nodes, lens, status = check(dev, points[:1], [cap], (200, 64), nb_points=8, slot=8)
    assert lens.tolist() == [[8, 0]]


def test_a_path_longer_than_its_slot(dev):
    shapes, size = P.hand_shapes()
    pix = dict((n, p) for n, p, _ in shapes)["three components, max_paths 2"]
    nodes, lens, status = check(dev, P.points_of_pixels(pix, 32)[None], [len(pix)], size, slot=5)
    assert status.tolist() == [2] and lens.tolist() == [[0, 5]] and (nodes[0, 0] == -1).all()


def test_refusals_leave_every_buffer_untouched(dev):
    pts, counts = np.zeros((2, 16), np.int32), [0, 0]
    cmax = L.lib().ivosw_robot_paths_max_cap()
    assert 4096 <= cmax and 36 * cmax + 256 <= 160 * 1024 < 36 * (cmax + 1) + 256
    cases = [(dict(points=None), "null points"), (dict(counts=None), "null counts"), (dict(nodes=None), "null nodes"),
             (dict(lens=None), "null lens"), (dict(status=None), "null status"), (dict(m=0), "m < 1"), (dict(cap=0), "cap 0 outside"),
             (dict(cap=cmax + 1), f"cap {cmax + 1} outside [1, {cmax}]"), (dict(H=0), "H outside [1, 65535]"), (dict(H=65536), "H outside"),
             (dict(W=0), "W outside [1, 65535]"), (dict(W=65536), "W outside"), (dict(min_nb_nodes=0), "min_nb_nodes < 1"),
             (dict(max_paths=0), "max_paths outside [1, 8]"), (dict(max_paths=9), "max_paths outside [1, 8]"), (dict(slot=0), "slot outside [1, cap]"),
             (dict(slot=17), "slot outside [1, cap]"), (dict(nb_points=9, slot=8), "nb_points > slot")]
    for over, word in cases:
        rc, msg, *_ = run(dev, pts, counts, (40, 70), over=over)
        assert rc == ERR_ARG and word in msg and msg.startswith("ivosw_robot_paths: "), (over, msg)


def pair(dev, H, W, seed, n_obj, zoom=1):
    """Device label maps (gt, pred) [2,H,W] with n_obj objects from blobs (``zoom``: every blob pixel a zoom x zoom block)."""
    gt, pred = np.zeros((2, H, W), np.uint8), np.zeros((2, H, W), np.uint8)
    h, w = -(-H // zoom), -(-W // zoom)
    big = lambda s: np.kron(rr.blob(h, w, s), np.ones((zoom, zoom), bool))[:H, :W]
    for f in range(2):
        for o in range(1, n_obj + 1):
            gt[f][big(seed + 10 * f + o)] = o
            pred[f][big(seed + 100 + 10 * f + o)] = o
    return torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)


@pytest.fixture(scope="module")
def big_pair(dev):
    return pair(dev, 480, 854, 5, 3, zoom=20)              # (skeletons of 1500 .. 3300 pixels: below cap = 4096)


def test_interact_device_paths_equal_host_paths(dev, big_pair):
    drew = 0
    for seed in range(4):
        gt, pred = pair(dev, 37, 70, seed, 2)
        for p in (pred, None):
            for kw in (dict(), dict(nb_points=None), dict(background=True, max_paths=3, min_nb_nodes=2)):
                host = R.interact(gt, p, 2, 1, **kw)
                assert R.interact(gt, p, 2, 1, paths="device", **kw) == host, (seed, kw)
                assert R.interact(gt, p, 2, 1, paths="host", **kw) == host
                drew += len(host)
    assert drew > 40
    gt, pred = big_pair
    host = R.interact(gt, pred, 3, 0, background=True)
    assert len(host) >= 4 and R.interact(gt, pred, 3, 0, background=True, paths="device") == host
    with pytest.raises(ValueError, match="paths must be 'host' or 'device'"):
        R.interact(gt, pred, 3, 0, paths="gpu")
    with pytest.raises(ValueError, match="more than cap = 8"):
        R.interact(gt, pred, 3, 0, cap=8, paths="device")
    with pytest.raises(ValueError, match="slot = 4"):
        R.interact(gt, pred, 3, 0, nb_points=None, slot=4, paths="device")
    dp = R.interact_device(gt, pred, 3, 0)
    assert dp.nodes.data_ptr() == dp.buf.data_ptr() and dp.status.data_ptr() == dp.buf.data_ptr() + 4 * (dp.buf.numel() - 3)
    assert dp.table(2).tolist() == [[(k * 2 + r) * 8, 8, o, 2] for k, o in enumerate((1, 2, 3)) for r in range(2)]


def test_interact_maps_equal_scribble_maps_of_the_host_paths(dev, big_pair):
    for seed in range(3):
        gt, pred = pair(dev, 37, 70, seed, 2)
        host = R.interact(gt, pred, 2, 1, nb_points=None)
        assert host
        for roi in (None, 5):
            for as_float in (False, True):
                for size in (None, (37, 70), (9, 17)):
                    want = S.scribble_maps({"scribbles": [host]}, size or (37, 70), roi_dist=roi, as_float=as_float)
                    maps, dp = R.interact_maps(gt, pred, 2, 1, size=size, roi_dist=roi, as_float=as_float, nb_points=None)
                    assert maps.dtype == want.dtype and torch.equal(maps, want), (seed, roi, as_float, size)
                    assert dp.to_scribbles() == host
    gt, pred = big_pair
    host = R.interact(gt, pred, 3, 0, background=True)
    maps, _ = R.interact_maps(gt, pred, 3, 0, background=True)
    assert torch.equal(maps, S.scribble_maps({"scribbles": [host]}, (480, 854))) and int((maps >= 0).sum()) > 0


def test_the_chain_records_no_synchronising_call(dev, big_pair):
    """The Python chain under torch's synchronisation guard (a synchronising tensor call raises), the C chain skeleton -> paths -> raster
    under launch-sequence capture (a synchronising HIP call would break the capture)."""
    gt, pred = big_pair
    R.interact_maps(gt, pred, 3, 0)                                # (the workspaces exist now)
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        dp = R.interact_device(gt, pred, 3, 0)
        maps, dp2 = R.interact_maps(gt, pred, 3, 0, roi_dist=5)
        low, _ = R.interact_maps(gt, pred, 3, 0, size=(120, 213))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(dev)
    host = R.interact(gt, pred, 3, 0)
    assert dp.to_scribbles() == host and torch.equal(low, S.scribble_maps({"scribbles": [host]}, (120, 213)))

    lib, m, cap, H, W = L.lib(), 3, 4096, 480, 854
    units = np.array([(0, 1), (0, 2), (0, 3)], np.int32)
    sk = torch.zeros(m * (2 + cap), dtype=torch.int32, device=dev)
    out = torch.zeros_like(dp.buf)
    n = m * 2 * 8 * 2
    table = dp.table(0)
    d_table = torch.from_numpy(table.reshape(-1)).to(dev)
    ws = torch.empty(lib.ivosw_scribble_raster_ws_bytes(1, H, W), dtype=torch.uint8, device=dev)
    drawn = torch.empty((1, H, W), dtype=torch.int8, device=dev)
    torch.cuda.synchronize(dev)
    with L.Graph.capture(dev) as g:
        st = L.stream_ptr(dev)
        L.check(lib.ivosw_robot_skeleton(L.dptr(gt), L.dptr(pred), 2, H, W, units.ctypes.data, m, cap, L.torch_ptr(sk, 2 * m), L.dptr(sk),
                                         L.torch_ptr(sk, m), None, st), "robot_skeleton")
        L.check(lib.ivosw_robot_paths(L.torch_ptr(sk, 2 * m), L.dptr(sk), m, cap, H, W, 4, 2, 8, 8, L.dptr(out), L.torch_ptr(out, n),
                                      L.torch_ptr(out, n + 2 * m), st), "robot_paths")
        L.check(lib.ivosw_scribble_raster(L.dptr(out), n // 2, L.dptr(d_table), table.ctypes.data, len(table), 1, H, W, -1, 1, -1,
                                          L.dptr(drawn), None, L.dptr(ws), ws.numel(), st), "scribble_raster")
    assert g.kernel_nodes >= 4, g.kernel_nodes                     # skeleton, paths, draw, finalise
    g.launch()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, dp.buf) and torch.equal(drawn, S.scribble_maps({"scribbles": [host]}, (H, W)))
