"""GPU: the boxed error-skeleton kernel (csrc/robot.hip, ivosw_robot_skeleton_box) - planes of the error region's bounding box only, in
LDS or in a global workspace, any frame size, object 0 - against the restatement of tests/robot_ref.py on the FULL frame: the bit plane,
the point list, the counts and the iteration counts bit for bit, on every pixel of every unit.

Every buffer (the workspace too) lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.  Each case
runs through the product entry (LDS window where the box fits) and through ivosw_robot_box_probe with 256 bytes of LDS (every non-empty box
on the global planes); the two must agree byte for byte with each other and, where ivosw_robot_skeleton accepts the call, with it."""
import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import robot as R
from tests import robot_ref as rr
from tests import test_gpu_robot as T

Buf, Call, FILL, ERR_ARG, blob = T.Buf, T.Call, T.FILL, T.ERR_ARG, rr.blob

pytestmark = pytest.mark.gpu

LDS_LIMIT, LDS_FIXED = 160 * 1024, 256
GLOBAL = 256                                              # the probe's budget that sends every non-empty box to the workspace


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class BoxCall(Call):
    """One ivosw_robot_skeleton_box call (``budget`` None) or one ivosw_robot_box_probe call with ``budget`` bytes of LDS, every buffer in
    guard bands.  The workspace is as large as the entry asks (and a token 64 bytes where it asks for none: they must stay untouched)."""

    def __init__(self, dev, gt, pred, units, cap, budget=None, **kw):
        super().__init__(dev, gt, pred, units, cap, **kw)
        self.budget = budget
        full = 2 * self.H * self.WW * 4 + LDS_FIXED
        self.need = max(self.m, 1) * 2 * self.H * self.WW * 4 if full > (min(full, LDS_LIMIT) if budget is None else budget) else 0
        self.b_ws = Buf(dev, np.full(max(self.need, 64) // 4, FILL, np.int32), FILL)

    def lib(self):
        return L.lib() if self.budget is None else L.probe_lib()

    def run(self, **over):
        a = dict(gt=self.b_gt.ptr(), pred=self.b_pred.ptr() if self.b_pred else None, n=self.n, H=self.H, W=self.W,
                 units=self.units.ctypes.data, m=self.m, cap=self.cap, points=self.b_points.ptr(), counts=self.b_counts.ptr(),
                 iters=self.b_iters.ptr(), skel=self.b_skel.ptr() if self.b_skel else None, ws=self.b_ws.ptr(), ws_bytes=max(self.need, 64))
        a.update(over)
        args = [a[k] for k in ("gt", "pred", "n", "H", "W", "units", "m", "cap", "points", "counts", "iters", "skel", "ws", "ws_bytes")]
        if self.budget is None:
            return L.lib().ivosw_robot_skeleton_box(*args, L.stream_ptr(self.dev))
        return L.probe_lib().ivosw_robot_box_probe(*args, self.budget, L.stream_ptr(self.dev))

    def outputs(self, unchanged=False):
        out = super().outputs(unchanged)
        self.b_ws.back("workspace", unchanged or self.need == 0)
        return out


def _refs(gt, pred, units, thin=rr.thin):
    """The restatement of every unit on the full frame: [(plane, skeleton, words, points, iters)], each distinct plane thinned once."""
    seen, out = {}, []
    for f, o in np.asarray(units).reshape(-1, 2).tolist():
        plane = rr.error_plane(gt[f], None if pred is None else pred[f], o)
        key = plane.tobytes()
        if key not in seen:
            sk, it = thin(plane)
            seen[key] = (sk, rr.pack_bits(sk), rr.points_of(sk), it)
        out.append((plane,) + seen[key])
    return out


def _check(call, refs, rc):
    """Every output of every unit against the restatement; returns the raw outputs."""
    assert rc == 0, call.lib().ivosw_last_error()
    points, counts, iters, skel = outs = call.outputs()
    for k, (plane, sk, words, pts, it) in enumerate(refs):
        if skel is not None:
            np.testing.assert_array_equal(skel[k], words, err_msg=f"unit {k} {call.units[k].tolist()}: bit plane")
        assert counts[k] == len(pts) and iters[k] == it, (k, call.units[k].tolist(), counts[k], len(pts), iters[k], it)
        kept = min(len(pts), call.cap)
        np.testing.assert_array_equal(points[k, :kept], pts[:kept], err_msg=f"unit {k}: points")
        assert (points[k, kept:] == FILL).all(), f"unit {k}: written behind its {kept} points"
        assert not (sk & ~plane).any()
    return outs


def _same(a, b, what):
    for x, y, name in zip(a, b, ("points", "counts", "iters", "skel")):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), f"{what}: {name} differ"


def _all_ways(dev, gt, pred, units, cap, refs, old=True, **kw):
    """Product entry, probe on the global planes and (``old``) ivosw_robot_skeleton on one case: each equals the restatement, all equal each
    other byte for byte."""
    box = BoxCall(dev, gt, pred, units, cap, **kw)
    a = _check(box, refs, box.run())
    glob = BoxCall(dev, gt, pred, units, cap, budget=GLOBAL, **kw)
    assert glob.need > 0
    b = _check(glob, refs, glob.run())
    _same(a, b, "LDS window and global planes")
    if old:
        call = Call(dev, gt, pred, units, cap, **kw)
        assert call.run() == 0, L.lib().ivosw_last_error()
        _same(a, call.outputs(), "box entry and ivosw_robot_skeleton")
    return a


# ------------------------------------------------------------------------------------------------ the window zoo
FH, FW = 41, 203                                          # the larger frame: an odd width and an odd frame stride, so every 16-byte phase occurs
PLACES = [(r, c) for r in (0, 5) for c in (0, 31, 37, 64)] + ["flush"]


@pytest.mark.parametrize("H", T.HEIGHTS)
@pytest.mark.parametrize("W", T.WIDTHS)
def test_window_zoo(dev, H, W):
    """Every shape of the existing zoo at (H, W), pasted into a 41 x 203 frame at every placement: the window's origin is not the frame's,
    its first word starts mid-word (columns 31, 37), the box touches the frame's edges (0, flush).  One unit per (shape, placement), each
    on a frame of its own behind an unused frame 0 (frame index > 0), as object 1 + k % 250 among other labels: 63 units at 1 x 1, more than 64 at every size
    with a 2 x 2 block, so the launch-group seam is crossed as well."""
    shapes = T._shapes(H, W)
    cases = [(name, p, place) for name, p in shapes.items() for place in PLACES]
    gt = np.zeros((len(cases) + 1, FH, FW), np.uint8)
    units = []
    for k, (name, p, place) in enumerate(cases):
        r, c = (FH - H, FW - W) if place == "flush" else place
        o = 1 + k % 250
        frame = ((o % 250) + 1) * (np.arange(FW)[None] % 3 == 0) * np.ones((FH, 1), int)             # another label on every third column
        frame[r:r + H, c:c + W] = np.where(p, o, frame[r:r + H, c:c + W])
        gt[k + 1] = frame
        units.append((k + 1, o))
    assert len(units) >= 63
    refs = _refs(gt, None, units)
    points, counts, iters, skel = _all_ways(dev, gt, None, units, H * W, refs)
    by_name = {}
    for (name, p, place), (plane, sk, _, pts, it) in zip(cases, refs):
        assert plane.sum() == p.sum()
        by_name.setdefault(name, set()).add((len(pts), it))
    assert all(len(v) == 1 for v in by_name.values()), by_name                        # a skeleton does not depend on where the shape lies
    assert by_name["empty"] == {(0, 0)}


def test_units_with_pred_and_every_phase(dev):
    """Several units in one launch with pred given, pred NULL, gt off the 16-byte grid and pred off gt's phase (the byte path of the box
    pass; phase A shifts gt and pred by their own byte phases)."""
    H, W = 21, 45
    rng = np.random.default_rng(11)
    gt = np.stack([np.where(blob(H, W, 20 + f), 1 + f % 2, np.where(blob(H, W, 30 + f), 7, 0)) for f in range(3)]).astype(np.uint8)
    pred = np.stack([np.roll(g, (2, -3), (0, 1)) for g in gt]).astype(np.uint8)
    pred[rng.random(pred.shape) < 0.02] = 255
    units = [(2, 1), (0, 1), (1, 2), (1, 7), (0, 7), (2, 7), (1, 1), (0, 255)]
    for kw, p in ((dict(), pred), (dict(), None), (dict(off=3), pred), (dict(off=0, pred_off=5), pred), (dict(off=1, pred_off=2), pred),
                  (dict(off=2, pred_off=2), pred)):
        refs = _refs(gt, p, units)
        _all_ways(dev, gt, p, units, 200, refs, **kw)
    box = BoxCall(dev, gt, None, [(1, 1)], 50, want_bits=False)                       # skel is optional
    _check(box, _refs(gt, None, [(1, 1)]), box.run())


# ------------------------------------------------------------------------------------------------ 720 x 1280
@pytest.fixture(scope="module")
def hd():
    """720 x 1280, frame 1: object 3 a missed disc of radius 100 off-centre (a 201-row x 8-word box: LDS); object 5 two blobs in opposite
    corners (the box is the whole frame, 230 KB: the workspace); object 7 a rectangle that the prediction has moved by 2 pixels (a 2-pixel
    sliver: one iteration).  The restatement (thin_fast: thin is per pixel and too slow here), once."""
    H, W = 720, 1280
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((2, H, W), np.uint8)
    gt[1][(yy - 300) ** 2 + (xx - 510) ** 2 <= 100 ** 2] = 3                          # columns 410 .. 610: words 12 .. 19
    gt[1, :24, :40][blob(24, 40, 3)] = 5
    gt[1, H - 24:, W - 40:][blob(24, 40, 4)] = 5
    gt[1, 0, :3] = gt[1, H - 1, W - 3:] = 5                                           # (whatever the blobs do: the first and the last pixel)
    gt[1, 500:560, 900:1000] = 7
    pred = np.zeros_like(gt)
    pred[1][np.roll(gt[1] == 7, 2, 1)] = 7
    units = [(1, 3), (1, 5), (1, 7)]
    refs = _refs(gt, pred, units, thin=rr.thin_fast)
    return gt, pred, units, refs


def test_720p_through_the_product_entry(dev, hd):
    gt, pred, units, refs = hd
    lib = L.lib()
    assert lib.ivosw_robot_skeleton_fits(720, 1280) == 0 and lib.ivosw_robot_box_workspace_bytes(720, 1280, 3) == 3 * 230400
    for (plane, sk, _, pts, it), rows, words in zip(refs, (201, 720, 60), (8, 40, 1)):
        ys, xs = np.nonzero(plane)
        assert ys.max() - ys.min() + 1 == rows and (xs.max() >> 5) - (xs.min() >> 5) + 1 == words
    assert 2 * 201 * 8 * 4 + 256 <= LDS_LIMIT < 2 * 720 * 40 * 4 + 256
    assert refs[0][4] > 50 and refs[2][4] == 1 and len(refs[2][3]) > 30              # the disc: many iterations; the sliver: exactly one
    box = BoxCall(dev, gt, pred, units, 4096)
    assert box.need == 3 * 2 * 720 * 40 * 4
    a = _check(box, refs, box.run())
    again = BoxCall(dev, gt, pred, units, 4096)
    assert again.run() == 0
    _same(a, again.outputs(), "two runs")
    # the disc alone forced onto the global planes gives the same bytes as its LDS window
    lds, glob = BoxCall(dev, gt, pred, units[:1], 4096), BoxCall(dev, gt, pred, units[:1], 4096, budget=GLOBAL)
    _same(_check(lds, refs[:1], lds.run()), _check(glob, refs[:1], glob.run()), "disc: LDS window and global planes")


def test_host_skeleton_points_at_720p(dev, hd):
    gt, pred, units, refs = hd
    assert not R.fits((720, 1280))
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    points, counts, iters, bits = R.skeleton_points(d_gt, d_pred, units, cap=2048, want_bits=True)
    assert points.is_cuda and tuple(points.shape) == (3, 2048) and tuple(bits.shape) == (3, 720, 40) and points.dtype == torch.int32
    assert points.data_ptr() == counts.data_ptr() + 2 * 3 * 4                         # still views of one buffer
    for k, (_, sk, words, pts, it) in enumerate(refs):
        assert int(counts[k]) == len(pts) and int(iters[k]) == it
        np.testing.assert_array_equal(points[k, :len(pts)].cpu().numpy(), pts)
        np.testing.assert_array_equal(bits[k].cpu().numpy().view(np.uint32), words)
    ws = dict(R._ws)
    assert (torch.device(dev), 3 * 2 * 720 * 40 * 4) in ws
    R.skeleton_points(d_gt, d_pred, units, cap=2048)
    assert list(R._ws) == list(ws) and all(R._ws[k] is ws[k] for k in ws)             # a steady session does not allocate


# ------------------------------------------------------------------------------------------------ object 0
def _two_objects(H, W, n=3):
    gt = np.stack([np.where(blob(H, W, 50 + f), 1, np.where(blob(H, W, 60 + f), 2, 0)) for f in range(n)]).astype(np.uint8)
    pred = np.stack([np.roll(g, (3, -4), (0, 1)) for g in gt]).astype(np.uint8)
    return gt, pred


def test_object_0_is_a_unit_like_any_other(dev):
    H, W = 33, 75
    gt, pred = _two_objects(H, W)
    for f in range(3):
        assert ((gt[f] == 0) & (pred[f] != 0)).sum() > 20                             # false positives exist
    units = [(1, 0), (1, 1), (1, 2), (2, 0), (0, 2), (0, 0)]
    refs = _refs(gt, pred, units)
    for k in (0, 3, 5):
        f = units[k][0]
        np.testing.assert_array_equal(refs[k][0], (gt[f] == 0) & (pred[f] != 0))
        assert refs[k][1].any()
    together = _all_ways(dev, gt, pred, units, 300, refs, old=False)
    for k, u in enumerate(units):                                                     # alone as in company
        alone = BoxCall(dev, gt, pred, [u], 300)
        one = _check(alone, refs[k:k + 1], alone.run())
        for x, y in zip(one, together):
            assert x[0].tobytes() == y[k].tobytes()
    many = [(k % 3, (k // 3) % 3) for k in range(70)]                                 # more than 64 units: the launch-group seam
    refs = _refs(gt, pred, many)
    out = _all_ways(dev, gt, pred, many, 300, refs, old=False, off=5)
    assert many[64][1] == 0 and out[1][64] > 0 and many[69][1] == 2


# ------------------------------------------------------------------------------------------------ refusals, overflow
def test_refusals_leave_every_buffer_alone(dev):
    gt = np.where(blob(9, 40, 1), 1, 0).astype(np.uint8)[None].repeat(2, 0)

    def units(rows):
        t = np.ascontiguousarray(np.asarray(rows, np.int32))
        return dict(units=t.ctypes.data, m=len(t), _keep=t)

    shared = [(dict(gt=None), "null gt"), (dict(points=None), "null points"), (dict(counts=None), "null counts"), (dict(iters=None), "null iters"),
              (dict(units=None), "null units_host"), (dict(m=0), "m < 1"), (dict(m=-2), "m < 1"), (dict(cap=0), "cap < 1"), (dict(n=0), "n < 1"),
              (dict(H=0), "H outside"), (dict(H=65536), "H outside"), (dict(W=0), "W outside"), (dict(W=-1), "W outside"), (dict(W=65536), "W outside"),
              (units([(0, 1), (2, 1)]), "unit 1: frame 2 outside [0, 2)"), (units([(-1, 1)]), "unit 0: frame -1 outside")]
    need = 3 * 2 * 720 * 40 * 4
    own = [(dict(H=720, W=1280, ws=None), f"needs {need} bytes"), (dict(H=720, W=1280, ws_bytes=need - 1), f"needs {need} bytes"),
           (dict(H=720, W=1280, ws=None, ws_bytes=need), "H = 720, W = 1280"),
           (units([(0, 1), (1, 1), (1, 0)]) | dict(pred=None), "unit 2: object 0"),
           (units([(0, 256)]), "unit 0: object 256 outside [0, 255]"), (units([(1, -1)]), "unit 0: object -1 outside [0, 255]")]
    for budget in (None, GLOBAL):
        for over, word in shared + own:
            if budget is not None and "H" in over and over["H"] == 720:
                continue                                                              # (the probe's small budget asks for another size)
            over = {k: v for k, v in over.items() if k != "_keep"}
            call = BoxCall(dev, gt, gt[::-1].copy(), [(0, 1), (1, 1), (1, 1)], 50, budget=budget)
            assert call.run(**over) == ERR_ARG, (over, call.lib().ivosw_last_error())
            assert word.encode() in call.lib().ivosw_last_error(), (word, call.lib().ivosw_last_error())
            call.outputs(unchanged=True)
    # the old entry's messages for the shared cases
    for over, word in shared:
        over = {k: v for k, v in over.items() if k != "_keep"}
        call = Call(dev, gt, gt[::-1].copy(), [(0, 1), (1, 1), (1, 1)], cap=50)
        assert call.run(**over) == ERR_ARG and word.encode() in L.lib().ivosw_last_error()
    # the probe: a workspace one byte short of what ITS budget asks, and budgets outside [256, 160 KB]
    call = BoxCall(dev, gt, None, [(0, 1), (1, 1)], 50, budget=GLOBAL)
    assert call.need == 2 * 2 * 9 * 2 * 4
    for over in (dict(ws=None), dict(ws_bytes=call.need - 1)):
        assert call.run(**over) == ERR_ARG and f"needs {call.need} bytes".encode() in L.probe_lib().ivosw_last_error()
    for bad in (255, 0, -1, LDS_LIMIT + 1):
        call.budget = bad
        assert call.run() == ERR_ARG and b"lds_budget_bytes" in L.probe_lib().ivosw_last_error()
    call.budget = GLOBAL
    call.outputs(unchanged=True)
    with pytest.raises(RuntimeError, match="object 0 .* null pred"):
        R.skeleton_points(torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), None, [(0, 0)])
    with pytest.raises(RuntimeError, match="object 300 outside"):
        R.skeleton_points(torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), [(0, 0), (0, 300)])


def test_overflow_keeps_the_count_true_and_writes_nothing_behind_cap(dev):
    H, W = 17, 96
    gt = np.zeros((1, H, W), np.uint8)
    gt[0, 3:6, 2:94] = 4                                                              # thins to a line of about 90 pixels
    gt[0, 10:13, 2:94] = 4
    refs = _refs(gt, None, [(0, 4), (0, 4)])
    n = len(refs[0][3])
    assert n > 150
    for cap in (1, 7, n - 1, n, n + 3):                                               # two units: unit 0 must not run into unit 1's row
        _all_ways(dev, gt, None, [(0, 4), (0, 4)], cap, refs)                         # (counts == n, FILL behind min(count, cap))


# ------------------------------------------------------------------------------------------------ the host functions
def test_interact_with_background_equals_the_restated_path_step(dev):
    H, W = 40, 70
    gt, pred = _two_objects(H, W, 2)
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    for kw in (dict(), dict(nb_points=None), dict(min_nb_nodes=8, max_paths=1, nb_points=3)):
        want = []
        for (_, sk, _, pts, _), o in zip(_refs(gt, pred, [(1, 0), (1, 1), (1, 2)]), (0, 1, 2)):
            want += rr.paths_from_points(pts, len(pts), (H, W), o, **kw)
        got = R.interact(d_gt, d_pred, 2, 1, background=True, **kw)
        assert got == want and got[0]["object_id"] == 0 and [q["object_id"] for q in got] == sorted(q["object_id"] for q in got)
        assert {q["object_id"] for q in got} == {0, 1, 2}
        assert R.interact(d_gt, d_pred, 2, 1, **kw) == [q for q in want if q["object_id"] != 0]
    # nothing predicted yet: no false positive exists, the background is skipped without error
    assert R.interact(d_gt, None, 2, 1, background=True) == R.interact(d_gt, None, 2, 1)
    assert R.interact(d_gt, d_gt.clone(), 2, 1, background=True) == []


def test_which_entry_the_host_calls(dev, monkeypatch):
    lib = L.lib()
    called = []
    old, box = lib.ivosw_robot_skeleton, lib.ivosw_robot_skeleton_box
    monkeypatch.setattr(lib, "ivosw_robot_skeleton", lambda *a: called.append("old") or old(*a))
    monkeypatch.setattr(lib, "ivosw_robot_skeleton_box", lambda *a: called.append("box") or box(*a))
    gt = torch.zeros(1, 480, 854, dtype=torch.uint8, device=dev)
    gt[0, 100:140, 200:300] = 1
    pred = torch.roll(gt, 3, 2)
    a = R.skeleton_points(gt, pred, [(0, 1)])
    R.interact(gt, pred, 1, 0)
    assert called == ["old", "old"]                                                   # 480p without the background: the old symbol, as before
    b = R.skeleton_points(gt, pred, [(0, 1), (0, 0)])
    R.interact(gt, pred, 1, 0, background=True)
    assert called[2:] == ["box", "box"]
    n = int(a[1][0])
    assert n == int(b[1][0]) > 0 and torch.equal(a[0][0, :n], b[0][0, :n]) and int(b[1][1]) > 0
    big = torch.zeros(1, 720, 1280, dtype=torch.uint8, device=dev)
    R.skeleton_points(big, None, [(0, 1)])
    assert called[4:] == ["box"]


# ------------------------------------------------------------------------------------------------ the option
def test_closed_loop_draws_background_scribbles_on_false_positives(dev, tmp_path, monkeypatch, capsys):
    """scribbles=paths robot=errors robot_background=true on the tiny session of tests/test_gpu_robot.py: from the second interaction on,
    every pixel the scribbles mark for a label o - 0 included - is a pixel of o in the ground truth where the masks submitted before
    differed from it; at least one interaction draws a background path (the stand-in shifts the masks of far frames by 1.5 pixels per
    frame of distance, and method=worst annotates a far frame: the strip the object moved into is background that was predicted as
    object, several pixels thick and tens long)."""
    from ivos_w_amd import entry
    from tests import scribble_ref as sr
    handed, submitted = [], []
    real_get, real_submit = entry.SyntheticSession.get_scribbles, entry.SyntheticSession.submit_masks

    def get(self, only_last=False):
        out = real_get(self, only_last)
        handed.append((out[1], self.drew, self.davis.load_annotations(out[0]).cpu().numpy()))
        return out

    def submit(self, masks, next_scribble_frame_candidates=None):
        submitted.append(torch.as_tensor(masks).cpu().numpy().copy())
        return real_submit(self, masks, next_scribble_frame_candidates)
    monkeypatch.setattr(entry.SyntheticSession, "get_scribbles", get)
    monkeypatch.setattr(entry.SyntheticSession, "submit_masks", submit)
    args = T.COMMON + [f"ckpt_dir={tmp_path}/weights", "scribbles=paths", "robot=errors", "robot_background=true",
                       f"report_save_dir={tmp_path}/bg"]
    out = entry.run_eval(entry.parse_cli(args), "MANet")
    text = capsys.readouterr().out
    assert len(handed) == 4 and len(out["curve"]["J_AND_F"]) == 4 and text.count("robot: ") == 4 and text.count(" background) ") == 4
    assert all(p["object_id"] != 0 for p in handed[0][0]["scribbles"][handed[0][0]["annotated_frame"]])      # nothing submitted yet
    drawn_bg = 0
    for k in range(1, 4):
        (sc, drew, gt), pred = handed[k], submitted[k - 1]
        f = sc["annotated_frame"]
        paths = sc["scribbles"][f]
        n_bg = sum(p["object_id"] == 0 for p in paths)
        print(f"interaction {k + 1}: frame {f}, robot {drew}, {len(paths)} paths, {n_bg} on the background, "
              f"false positives {int(((gt[f] == 0) & (pred[f] != 0)).sum())}")
        assert drew == "errors" and f"robot: errors ({n_bg} background)" in text
        assert [p["object_id"] for p in paths] == sorted(p["object_id"] for p in paths)
        full = sr.scribbles2mask(sc, gt.shape[1:])[f]
        ys, xs = np.nonzero(full >= 0)
        assert (gt[f][ys, xs] == full[ys, xs]).all() and (pred[f][ys, xs] != full[ys, xs]).all()
        only_bg = sr.scribbles2mask(dict(sc, scribbles=[[p for p in per if p["object_id"] == 0] for per in sc["scribbles"]]), gt.shape[1:])[f]
        ys, xs = np.nonzero(only_bg == 0)
        assert len(ys) >= 4 * n_bg and (gt[f][ys, xs] == 0).all() and (pred[f][ys, xs] != 0).all()
        drawn_bg += n_bg
    assert drawn_bg >= 1
