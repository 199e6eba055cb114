"""GPU: the error-skeleton kernel (csrc/robot.hip) through the C ABI and through utils/robot.py against the per-pixel restatement of
tests/robot_ref.py: the bit plane, the point list, the counts and the iteration counts bit for bit, on every pixel of every case.

Every buffer lies inside a guard band whose fill must survive; a refused call leaves every buffer as it was.  The widths walk the word
carries (31 / 32 / 33, 63 / 64 / 65) and, with a frame index > 0 and odd widths, every phase of the 16-byte loads of the error plane."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import robot as R
from tests import robot_ref as rr

EIGHT, blob = rr.EIGHT, rr.blob

pytestmark = pytest.mark.gpu

PAD = 16                                                  # elements in front of and behind every buffer
FILL = -7                                                 # int32 outputs; the uint32 plane shows it as 0xfffffff9
ERR_ARG = -1
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 96)
HEIGHTS = (1, 2, 3, 17)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class Buf:
    """A device buffer holding ``data`` (flat) PAD + off elements inside an allocation filled with ``fill``; ``back()`` returns the data as
    it is now after checking the guard bands."""

    def __init__(self, dev, data, fill, off=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.lo, self.n = PAD + off, data.size
        self.host = np.full(data.size + 3 * PAD, fill, data.dtype)
        self.host[self.lo:self.lo + self.n] = data
        self.t = torch.from_numpy(self.host).to(dev)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.lo * self.t.element_size())

    def back(self, name, unchanged=False):
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == self.host[:self.lo]).all() and (h[self.lo + self.n:] == self.host[self.lo + self.n:]).all(), \
            f"{name}: written outside its extent"
        if unchanged:
            np.testing.assert_array_equal(h, self.host, err_msg=f"{name}: written by a refused call / an input")
        return h[self.lo:self.lo + self.n]


class Call:
    """One ivosw_robot_skeleton call with every buffer in guard bands; keyword overrides replace single C arguments.  ``off`` moves gt
    (and ``pred_off`` pred) by that many bytes off the 16-byte grid."""

    def __init__(self, dev, gt, pred, units, cap, off=0, pred_off=None, want_bits=True):
        self.gt = np.ascontiguousarray(gt, np.uint8)
        self.n, self.H, self.W = self.gt.shape
        self.WW = (self.W + 31) // 32
        self.units = np.ascontiguousarray(np.asarray(units, np.int32).reshape(-1, 2))
        self.m, self.cap, self.dev = len(self.units), cap, dev
        self.b_gt = Buf(dev, self.gt, 201, off)
        self.b_pred = None if pred is None else Buf(dev, np.ascontiguousarray(pred, np.uint8), 202, off if pred_off is None else pred_off)
        m = max(self.m, 1)
        self.b_points = Buf(dev, np.full(m * max(cap, 1), FILL, np.int32), FILL)
        self.b_counts = Buf(dev, np.full(m, FILL, np.int32), FILL)
        self.b_iters = Buf(dev, np.full(m, FILL, np.int32), FILL)
        self.b_skel = Buf(dev, np.full(m * self.H * self.WW, FILL, np.int32), FILL) if want_bits else None

    def run(self, **over):
        a = dict(gt=self.b_gt.ptr(), pred=self.b_pred.ptr() if self.b_pred else None, n=self.n, H=self.H, W=self.W,
                 units=self.units.ctypes.data, m=self.m, cap=self.cap, points=self.b_points.ptr(), counts=self.b_counts.ptr(),
                 iters=self.b_iters.ptr(), skel=self.b_skel.ptr() if self.b_skel else None)
        a.update(over)
        return L.lib().ivosw_robot_skeleton(a["gt"], a["pred"], a["n"], a["H"], a["W"], a["units"], a["m"], a["cap"], a["points"],
                                            a["counts"], a["iters"], a["skel"], L.stream_ptr(self.dev))

    def outputs(self, unchanged=False):
        """(points [m,cap], counts [m], iters [m], skel uint32 [m,H,WW] or None) after the guard bands of EVERY buffer were checked."""
        self.b_gt.back("gt", unchanged=True)
        if self.b_pred:
            self.b_pred.back("pred", unchanged=True)
        points = self.b_points.back("points", unchanged).reshape(max(self.m, 1), -1)
        counts, iters = self.b_counts.back("counts", unchanged), self.b_iters.back("iters", unchanged)
        skel = self.b_skel.back("skel", unchanged).view(np.uint32).reshape(max(self.m, 1), self.H, self.WW) if self.b_skel else None
        return points, counts, iters, skel


_REF = {}


def _ref(gt, pred, frame, obj):
    """The restatement of one unit, computed once per distinct error plane."""
    plane = rr.error_plane(gt[frame], None if pred is None else pred[frame], obj)
    key = (plane.shape, plane.tobytes())
    if key not in _REF:
        sk, iters = rr.thin(plane)
        _REF[key] = (sk, rr.pack_bits(sk), rr.points_of(sk), iters)
    return (plane,) + _REF[key]


def _check(call, pred, rc):
    """Every output of every unit against the restatement; returns the per-unit (skeleton, iters)."""
    assert rc == 0, L.lib().ivosw_last_error()
    points, counts, iters, skel = call.outputs()
    out = []
    for k, (f, o) in enumerate(call.units.tolist()):
        plane, sk, words, pts, it = _ref(call.gt, pred, f, o)
        if skel is not None:
            np.testing.assert_array_equal(skel[k], words, err_msg=f"unit {k}: bit plane")
        assert counts[k] == len(pts) and iters[k] == it, (k, counts[k], len(pts), iters[k], it)
        kept = min(len(pts), call.cap)
        np.testing.assert_array_equal(points[k, :kept], pts[:kept], err_msg=f"unit {k}: points")
        assert (points[k, kept:] == FILL).all(), f"unit {k}: written behind its {kept} points"
        assert not (sk & ~plane).any()
        out.append((sk, it))
    return out


def _shapes(H, W):
    """The shape zoo of one size as {name: bool plane}."""
    z = lambda: np.zeros((H, W), bool)
    out = {"empty": z(), "ones": np.ones((H, W), bool)}
    for name, x0 in (("bar31", 29), ("bar63", 61)):                       # bars across the word seams 31 | 32 and 63 | 64
        if W > x0 + 5:
            p = z()
            p[max(H // 2 - 1, 0):H // 2 + 2, x0:x0 + 6] = True
            out[name] = p
    if H >= 7 and W >= 7:
        p = z()
        p[1:H - 1, 1:W - 1] = True
        p[3:H - 3, 3:W - 3] = False
        out["ring"] = p
    p = z()
    for k in range(min(H, W)):
        p[k, k] = True
    out["diag1"] = p
    p = p.copy()
    for k in range(min(H, W - 1)):
        p[k, k + 1] = True
    out["diag2"] = p
    if H >= 2 and W >= 2:
        p = z()
        p[H - 2:, W - 2:] = True
        out["block"] = p
    for seed in (0, 1, 2):
        out[f"blob{seed}"] = blob(H, W, seed)
    return out


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_skeleton_equals_the_restatement(dev, H, W):
    """Every shape of the zoo as its own object of one frame stack: frame k holds shape k as object k + 1 among other labels, pred is NULL.
    "ones" is the filled rectangle that touches all four borders.  One launch for all shapes."""
    shapes = _shapes(H, W)
    gt = np.zeros((len(shapes), H, W), np.uint8)
    for k, p in enumerate(shapes.values()):
        gt[k] = np.where(p, k + 1, (k + 2) * (np.arange(W)[None] % 3 == 0))          # other labels around it
    units = [(k, k + 1) for k in range(len(shapes))]
    call = Call(dev, gt, None, units, cap=H * W)
    got = dict(zip(shapes, _check(call, None, call.run())))
    assert got["empty"][1] == 0 and not got["empty"][0].any()
    if "block" in got:
        assert not got["block"][0].any()                                             # an isolated 2 x 2 block is deleted whole
    assert got["diag1"][0].sum() == min(H, W)                                        # a one-pixel diagonal is a skeleton already
    # as many 8-connected components as the region, on the shapes that hold no 2 x 2-only component
    for name in ("ones", "ring", "bar31", "bar63", "diag1", "diag2"):
        if name in got and not (name == "ones" and (H, W) == (2, 2)):
            assert ndimage.label(got[name][0], EIGHT)[1] == ndimage.label(shapes[name], EIGHT)[1], name


def test_units_of_one_launch_with_and_without_pred(dev):
    """Several units in one launch: different frames and objects of a 3-frame stack of odd width (every 16-byte phase of the rows, a
    ragged head and tail per frame), pred given, pred NULL, and pred off gt's 16-byte phase (the byte path)."""
    H, W = 21, 45
    rng = np.random.default_rng(11)
    gt = np.stack([np.where(blob(H, W, 20 + f), 1 + f % 2, np.where(blob(H, W, 30 + f), 7, 0)) for f in range(3)]).astype(np.uint8)
    pred = np.stack([np.roll(g, (2, -3), (0, 1)) for g in gt]).astype(np.uint8)
    pred[rng.random(pred.shape) < 0.02] = 255
    units = [(2, 1), (0, 1), (1, 2), (1, 7), (0, 7), (2, 7), (1, 1), (0, 255)]          # (1, 1): an object the frame does not hold
    for kw, p in ((dict(), pred), (dict(), None), (dict(off=3), pred), (dict(off=0, pred_off=5), pred)):
        call = Call(dev, gt, p, units, cap=200, **kw)
        got = _check(call, p, call.run())
        assert got[0][0].any() and not got[6][0].any() and got[6][1] == 0
    # the same planes through the host function
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    points, counts, iters, bits = R.skeleton_points(d_gt, d_pred, units, cap=200, want_bits=True)
    assert points.is_cuda and tuple(points.shape) == (8, 200) and tuple(bits.shape) == (8, H, 2) and points.dtype == torch.int32
    for k, (f, o) in enumerate(units):
        _, sk, words, pts, it = _ref(gt, pred, f, o)
        assert int(counts[k]) == len(pts) and int(iters[k]) == it
        np.testing.assert_array_equal(points[k, :len(pts)].cpu().numpy(), pts)
        np.testing.assert_array_equal(bits[k].cpu().numpy().view(np.uint32), words)


def test_sixty_five_units_run_in_two_groups(dev):
    H, W = 9, 40
    gt = np.stack([np.where(blob(H, W, 40 + f), 1, 2) for f in range(5)]).astype(np.uint8)
    units = [(k % 5, 1 + (k // 5) % 2) for k in range(65)]
    call = Call(dev, gt, None, units, cap=64)
    got = _check(call, None, call.run())
    assert len(got) == 65 and got[64][0].any()


@pytest.fixture(scope="module")
def full_size():
    """480 x 854, a disc of radius 100: the restatement, once."""
    yy, xx = np.mgrid[:480, :854]
    gt = np.zeros((2, 480, 854), np.uint8)
    gt[1][(yy - 250) ** 2 + (xx - 411) ** 2 <= 100 ** 2] = 3
    return gt


def test_full_size_plane(dev, full_size):
    """The LDS-limit path of the robot's own size: 103 936 bytes of dynamic LDS, 27 words per row, rows of 854 bytes (2-byte phase)."""
    assert L.lib().ivosw_robot_skeleton_fits(480, 854) == 1 and L.lib().ivosw_robot_skeleton_fits(720, 1280) == 0
    call = Call(dev, full_size, None, [(1, 3)], cap=4096)
    ((sk, it),) = _check(call, None, call.run())
    assert it > 50 and sk.any() and ndimage.label(sk, EIGHT)[1] == 1
    again = Call(dev, full_size, None, [(1, 3)], cap=4096)
    assert again.run() == 0
    for a, b in zip(call.outputs(), again.outputs()):                                 # two runs give identical bits
        assert a.tobytes() == b.tobytes()


def test_largest_size_runs_and_the_next_is_refused(dev):
    lib = L.lib()
    W = 40                                                                            # two words per row
    H = max(h for h in range(1, 65536) if 2 * h * 2 * 4 + 256 <= 160 * 1024)
    assert H == 10224 and lib.ivosw_robot_skeleton_fits(H, W) == 1 and lib.ivosw_robot_skeleton_fits(H + 1, W) == 0
    assert lib.ivosw_robot_skeleton_fits(0, 5) == 0 and lib.ivosw_robot_skeleton_fits(5, 65536) == 0
    gt = np.zeros((1, H + 1, W), np.uint8)
    gt[0, 5:H - 5, 30:35] = 1                                                         # a tall bar across the seam, down to the last rows
    gt[0, H - 2:H, 0:3] = 1
    call = Call(dev, gt[:, :H], None, [(0, 1)], cap=H)
    ((sk, it),) = _check(call, None, call.run())
    assert sk.sum() > H - 40 and it >= 2
    call = Call(dev, gt, None, [(0, 1)], cap=H)
    assert call.run() == ERR_ARG
    msg = lib.ivosw_last_error().decode()
    assert f"H = {H + 1}" in msg and f"W = {W}" in msg and "163840" in msg, msg
    call.outputs(unchanged=True)


def test_refusals_leave_every_buffer_alone(dev):
    lib = L.lib()
    gt = np.where(blob(9, 40, 1), 1, 0).astype(np.uint8)[None].repeat(2, 0)

    def units(rows):
        t = np.ascontiguousarray(np.asarray(rows, np.int32))
        return dict(units=t.ctypes.data, m=len(t), _keep=t)

    cases = [(dict(gt=None), "null gt"), (dict(points=None), "null points"), (dict(counts=None), "null counts"), (dict(iters=None), "null iters"),
             (dict(units=None), "null units_host"), (dict(m=0), "m < 1"), (dict(m=-2), "m < 1"), (dict(cap=0), "cap < 1"), (dict(n=0), "n < 1"),
             (dict(H=0), "H outside"), (dict(H=65536), "H outside"), (dict(W=0), "W outside"), (dict(W=-1), "W outside"), (dict(W=65536), "W outside"),
             (dict(H=720, W=1280), "H = 720, W = 1280"),
             (units([(0, 1), (2, 1)]), "unit 1: frame 2 outside [0, 2)"), (units([(-1, 1)]), "unit 0: frame -1 outside"),
             (units([(0, 1), (1, 1), (1, 0)]), "unit 2: object 0 outside [1, 255]"), (units([(0, 256)]), "unit 0: object 256 outside")]
    for over, word in cases:
        over = {k: v for k, v in over.items() if k != "_keep"}
        call = Call(dev, gt, gt[::-1].copy(), [(0, 1), (1, 1), (1, 1)], cap=50)
        assert call.run(**over) == ERR_ARG, (over, lib.ivosw_last_error())
        assert word.encode() in lib.ivosw_last_error(), (word, lib.ivosw_last_error())
        call.outputs(unchanged=True)
    # skel is optional, pred is optional
    call = Call(dev, gt, None, [(1, 1)], cap=50, want_bits=False)
    _check(call, None, call.run())
    with pytest.raises(TypeError, match="uint8 label map"):
        R.skeleton_points(torch.zeros(1, 4, 4, device=dev), None, [(0, 1)])
    with pytest.raises(RuntimeError, match="object 300 outside"):
        R.skeleton_points(torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), None, [(0, 300)])


def test_overflow_keeps_the_count_true_and_writes_nothing_behind_cap(dev):
    H, W = 17, 96
    gt = np.zeros((1, H, W), np.uint8)
    gt[0, 3:6, 2:94] = 4                                                              # thins to a line of about 90 pixels
    gt[0, 10:13, 2:94] = 4
    _, sk, _, pts, _ = _ref(gt, None, 0, 4)
    assert len(pts) > 150
    for cap in (1, 7, len(pts) - 1, len(pts), len(pts) + 3):
        call = Call(dev, gt, None, [(0, 4), (0, 4)], cap=cap)                          # two units: unit 0 must not run into unit 1's row
        _check(call, None, call.run())                                                # (counts == len(pts), FILL behind min(count, cap))
    d_gt = torch.from_numpy(gt).to(dev)
    with pytest.raises(ValueError, match=rf"unit 3 \(frame 0, object 4\).*{len(pts)} pixels.*cap = 16"):
        R.interact(d_gt, None, 4, 0, cap=16)


def test_interact_equals_the_restated_path_step(dev):
    H, W = 40, 70
    gt = np.zeros((2, H, W), np.uint8)
    gt[1][blob(H, W, 5)] = 1
    gt[1][blob(H, W, 6) & (gt[1] == 0)] = 2
    gt[1, 0, 0] = 3                                                                   # a single pixel: a skeleton below min_nb_nodes
    pred = np.roll(gt, 3, 2)
    d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    for p, d_p in ((None, None), (pred, d_pred)):
        for kw in (dict(), dict(nb_points=None), dict(min_nb_nodes=8, max_paths=1, nb_points=3)):
            want = []
            for o in (1, 2, 3):
                _, sk, _, pts, _ = _ref(gt, p, 1, o)
                want += rr.paths_from_points(pts, len(pts), (H, W), o, **kw)
            got = R.interact(d_gt, d_p, 3, 1, **kw)
            assert got == want and len(got) >= 2 and [q["object_id"] for q in got] == sorted(q["object_id"] for q in got)
            assert all(q["object_id"] != 3 for q in got)
    assert R.interact(d_gt, d_gt.clone(), 3, 1) == [] and R.interact(d_gt, None, 0, 1) == []


# ================================================================================================ the option
# method=worst annotates the frame with the lowest J&F next: far from every annotated frame, where the stand-in's shifted masks leave error
# regions of a hundred pixels and more (with method=ours and untrained weights the session may return to a frame that is almost right,
# whose few error pixels carry no path of min_nb_nodes pixels - the case the session answers with the ground-truth robot)
COMMON = ["with", "synthetic=1", "setting=oracle", "method=worst", "seed=0", "synth.n_sequences=1", "synth.n_frames=16", "synth.height=48",
          "synth.width=64", "eval_max_nb_interactions=4"]


def test_closed_loop_scribbles_lie_on_the_errors(dev, tmp_path, monkeypatch, capsys):
    """scribbles=paths robot=errors on one tiny sequence: from the second interaction on, every pixel the session's scribbles mark for
    an object o on the annotated frame - drawn at full resolution by the rasteriser's definition, and at the stand-in's stride-4
    resolution as run_eval draws them - is a pixel of o in the ground truth where the masks submitted before differed from it."""
    from ivos_w_amd import entry
    from tests import scribble_ref as sr
    handed, submitted, lows = [], [], []
    real_get, real_submit, real_logits = entry.SyntheticSession.get_scribbles, entry.SyntheticSession.submit_masks, entry.StandInVOS.logits

    def get(self, only_last=False):
        out = real_get(self, only_last)
        handed.append((out[1], self.drew, self.davis.load_annotations(out[0]).cpu().numpy()))
        return out

    def submit(self, masks, next_scribble_frame_candidates=None):
        submitted.append(torch.as_tensor(masks).cpu().numpy().copy())
        return real_submit(self, masks, next_scribble_frame_candidates)

    def logits(self, gt_u8, n_objects, annotated_frames, scribble_low=None):
        lows.append(scribble_low)
        return real_logits(self, gt_u8, n_objects, annotated_frames, scribble_low=scribble_low)
    monkeypatch.setattr(entry.SyntheticSession, "get_scribbles", get)
    monkeypatch.setattr(entry.SyntheticSession, "submit_masks", submit)
    monkeypatch.setattr(entry.StandInVOS, "logits", logits)
    args = COMMON + [f"ckpt_dir={tmp_path}/weights", "scribbles=paths", "robot=errors", f"report_save_dir={tmp_path}/errors"]
    out = entry.run_eval(entry.parse_cli(args), "MANet")
    text = capsys.readouterr().out
    assert len(handed) == len(lows) == 4 and len(out["curve"]["J_AND_F"]) == 4 and text.count("robot: ") == 4
    assert handed[0][1] == "errors" and text.count("robot: errors") == sum(h[1] == "errors" for h in handed)
    checked = 0
    for k in range(1, 4):
        (sc, drew, gt), pred = handed[k], submitted[k - 1]
        f = sc["annotated_frame"]
        print(f"interaction {k + 1}: frame {f}, robot {drew}, {len(sc['scribbles'][f])} paths, "
              f"error pixels per object {[int(((gt[f] == o) & (pred[f] != o)).sum()) for o in range(1, int(gt.max()) + 1)]}")
        assert drew == "errors", f"interaction {k + 1}: the error robot found no path"
        full = sr.scribbles2mask(sc, gt.shape[1:])[f]
        ys, xs = np.nonzero(full >= 0)
        assert len(ys) >= 4
        assert (gt[f][ys, xs] == full[ys, xs]).all() and (pred[f][ys, xs] != full[ys, xs]).all()
        frame, low = lows[k]
        low = low.cpu().numpy()
        np.testing.assert_array_equal(low, sr.scribbles2mask(sc, (12, 16))[f])
        for y, x in zip(*np.nonzero(low >= 0)):                                       # the 4 x 4 block of a marked stride-4 pixel holds such a pixel
            o = low[y, x]
            block = (gt[f, 4 * y:4 * y + 4, 4 * x:4 * x + 4] == o) & (pred[f, 4 * y:4 * y + 4, 4 * x:4 * x + 4] != o)
            assert block.any()
        checked += 1
    assert checked == 3
    # the first scribbles: nothing submitted yet, the error region is the object
    sc, drew, gt = handed[0]
    f = sc["annotated_frame"]
    full = sr.scribbles2mask(sc, gt.shape[1:])[f]
    assert (full >= 0).any() and (gt[f][full >= 0] == full[full >= 0]).all()


def test_robot_gt_is_the_default_run(dev, tmp_path, monkeypatch, capsys):
    from ivos_w_amd import entry
    monkeypatch.setattr(R, "interact", lambda *a, **k: pytest.fail("robot=gt called the error robot"))
    base = COMMON + [f"ckpt_dir={tmp_path}/weights", "scribbles=paths"]
    a = entry.run_eval(entry.parse_cli(base + [f"report_save_dir={tmp_path}/a"]), "MANet")
    text_a = capsys.readouterr().out
    b = entry.run_eval(entry.parse_cli(base + ["robot=gt", f"report_save_dir={tmp_path}/b"]), "MANet")
    text_b = capsys.readouterr().out
    assert a["auc"] == b["auc"] and a["curve"] == b["curve"] and "robot: " not in text_a and "robot: " not in text_b
    strip = lambda t: [ln.split("rec_time")[0] + ln.split("ms", 1)[-1] for ln in t.splitlines() if ln.startswith("avg_")]
    assert strip(text_a) == strip(text_b) and len(strip(text_a)) == 4
