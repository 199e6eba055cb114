"""GPU: J / F for several videos in one pass (ivosw_jf_counts_videos), the ratios and means on the device (ivosw_jf_reduce_ragged) and
the oracle chain on top (metrics.jf_videos, misc.sequence_metric_videos, utils_agent.oracle_recommend).  Bit equality throughout: the
counts against ivosw_jf_counts per video, everything behind them against the host path (tests/jf_videos_ref.py, sequence_metric,
recommend_frame / recommend_candidates)."""
import copy
import random

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import metrics, synth
from ivos_w_amd.models.agent import Agent, Brain
from ivos_w_amd.utils import misc, utils_agent
from tests import jf_videos_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -7


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    return L.lib()


# ---------------------------------------------------------------------------------------------- videos
def _labels(rng, n, H, W, n_ids, ids, mode="both"):
    """gt, pred uint8 [n,H,W]: blocky random labels over `ids` and background; pred = gt shifted, with some pixels redrawn."""
    values = np.array([0] + list(ids), dtype=np.uint8)
    cell = max(1, min(H, W) // 3)
    coarse = rng.integers(0, len(values), (n, -(-H // cell), -(-W // cell)))
    gt = values[np.kron(coarse, np.ones((1, cell, cell), dtype=np.int64))[:, :H, :W]]
    pred = np.roll(gt, (1, -2), axis=(1, 2)).copy()
    flip = rng.random((n, H, W)) < 0.05
    pred[flip] = values[rng.integers(0, len(values), int(flip.sum()))]
    if mode in ("no_pred", "neither"):
        pred[:] = 0
    if mode in ("no_gt", "neither"):
        gt[:] = 0
    return np.ascontiguousarray(gt), np.ascontiguousarray(pred)


def _derived(H, W):
    return int(metrics.bound_pixels((H, W)))


class _Vid:
    def __init__(self, dev, rng, n, H, W, ids, bp=None, mode="both"):
        self.n, self.H, self.W, self.ids = n, H, W, list(ids)
        self.bp = _derived(H, W) if bp is None else bp
        gt, pred = _labels(rng, n, H, W, len(self.ids), self.ids, mode)
        self.gt, self.pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)

    def desc(self):
        d = L.JfVideo(gt=self.gt.data_ptr(), pred=self.pred.data_ptr(), n_frames=self.n, H=self.H, W=self.W, n_obj=len(self.ids), bound_pix=self.bp)
        for i, v in enumerate(self.ids):
            d.obj_ids[i] = v
        return d


def _single_counts(lib, dev, v):
    counts = torch.empty(v.n, len(v.ids), 6, dtype=torch.int64, device=dev)
    nbytes = lib.ivosw_jf_ws_bytes(v.n, v.H, v.W, len(v.ids))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.ivosw_jf_counts(L.dptr(v.gt), L.dptr(v.pred), v.n, v.H, v.W, bytes(v.ids), len(v.ids), v.bp, L.dptr(counts), L.dptr(ws), nbytes,
                                L.stream_ptr(dev)), "jf_counts")
    return counts


def _videos_counts(lib, dev, vids):
    table = (L.JfVideo * len(vids))(*[v.desc() for v in vids])
    total = sum(v.n * len(v.ids) * 6 for v in vids)
    nbytes = lib.ivosw_jf_videos_ws_bytes(table, len(vids))
    assert nbytes == sum(lib.ivosw_jf_ws_bytes(v.n, v.H, v.W, len(v.ids)) for v in vids)
    counts = torch.full((total + 6,), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.ivosw_jf_counts_videos(table, len(vids), L.dptr(counts), L.dptr(ws), nbytes, L.stream_ptr(dev)), "jf_counts_videos")
    assert bool((counts[total:] == SENTINEL).all())
    return counts[:total]


def _assert_counts_equal(lib, dev, vids):
    got = _videos_counts(lib, dev, vids).cpu().numpy()
    off, nonzero = 0, 0
    for k, v in enumerate(vids):
        want = _single_counts(lib, dev, v).cpu().numpy().reshape(-1)
        np.testing.assert_array_equal(got[off:off + want.size], want, err_msg=f"video {k}: {v.n}x{v.H}x{v.W}, ids {v.ids}, bound_pix {v.bp}")
        nonzero += int((want != 0).sum())
        off += want.size
    assert off == got.size and nonzero > 0


# ---------------------------------------------------------------------------------------------- counts
def test_counts_at_the_column_edges(lib, dev):
    """lane = 16 pixels, bitmap word = 32, wave segment = 1024: W around each; the smallest video first and again last, beside the widest."""
    rng = np.random.default_rng(1)
    widths = [1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025]
    vids = [_Vid(dev, rng, 1 + i % 2, 5 + i, W, [1 + i % 3, 4], bp=[None, 0, 1][i % 3]) for i, W in enumerate(widths)]
    vids.append(_Vid(dev, rng, 1, 1, 1, [2], bp=0))
    vids.insert(0, _Vid(dev, rng, 1, 1, 1, [1], bp=1))
    _assert_counts_equal(lib, dev, vids)
    _assert_counts_equal(lib, dev, vids[::-1])


def test_counts_at_the_row_edges_objects_and_tolerances(lib, dev):
    """A workgroup walks 16 rows (4 waves x 4 rows): H one below / at / above 16 and 32; 1 and 32 objects; bound_pix 0, 1, derived, 8, 32;
    different ids per video; all-background pred, gt, and both; a 1-frame video; the smallest video first and last beside the tallest."""
    rng = np.random.default_rng(2)
    all32 = list(range(32, 0, -1))
    vids = [_Vid(dev, rng, 1, 1, 3, [5], bp=1),
            _Vid(dev, rng, 2, 15, 40, [1, 2], bp=0), _Vid(dev, rng, 1, 16, 33, [3], bp=1), _Vid(dev, rng, 3, 17, 40, [2, 1, 7]),
            _Vid(dev, rng, 1, 31, 20, all32, bp=1), _Vid(dev, rng, 2, 32, 17, [9]), _Vid(dev, rng, 1, 33, 70, all32, bp=8),
            _Vid(dev, rng, 2, 20, 24, [1, 2], mode="no_pred"), _Vid(dev, rng, 2, 20, 24, [2, 1], mode="no_gt"),
            _Vid(dev, rng, 1, 9, 40, [1], mode="neither"), _Vid(dev, rng, 2, 40, 90, [1, 2, 3], bp=32),
            _Vid(dev, rng, 1, 70, 300, [4, 1]), _Vid(dev, rng, 1, 1, 1, [1], bp=0)]
    assert _derived(70, 300) == 3 and _derived(17, 40) == 1
    _assert_counts_equal(lib, dev, vids)
    _assert_counts_equal(lib, dev, vids[::-1])
    _assert_counts_equal(lib, dev, [vids[6]])                             # one video through the table path


def test_a_full_table_of_videos(lib, dev):
    rng = np.random.default_rng(3)
    vids = [_Vid(dev, rng, 1 + k % 3, 3 + (5 * k) % 37, 2 + (11 * k) % 75, [1 + k % 4, 6][:1 + k % 2]) for k in range(L.MAX_JF_VIDEOS)]
    _assert_counts_equal(lib, dev, vids)


# ---------------------------------------------------------------------------------------------- reduce
@pytest.fixture(scope="module")
def hand_counts():
    """The hand-made counts of the CPU list, one 'video' per object count, and the host path's answers, computed once."""
    vids = [R.make_counts(R.min_frames(o) + i % 3, o, seed=o) for i, o in enumerate(R.OBJECT_COUNTS)]
    vids.insert(3, R.make_counts(1, 4, seed=40))                          # a one-frame sequence
    want = {(m, avg): [R.host_metric(c, m, avg) for c in vids] for m in R.METRICS for avg in (True, False)}
    return vids, want


def _reduce(lib, dev, vids, metric, per_obj, state):
    n_obj, lengths = [c.shape[1] for c in vids], [c.shape[0] for c in vids]
    rows, pairs = sum(lengths), sum(c.shape[0] * c.shape[1] for c in vids)
    counts = torch.from_numpy(np.concatenate([c.reshape(-1) for c in vids])).to(dev)
    quality = torch.full((rows + 1,), float(SENTINEL), dtype=torch.float64, device=dev)
    per = torch.full((pairs + 1,), float(SENTINEL), dtype=torch.float64, device=dev) if per_obj else None
    annot = torch.arange(rows, dtype=torch.float32, device=dev) % 5 if state else None
    st = torch.full((rows + 1, 2), float(SENTINEL), dtype=torch.float32, device=dev) if state else None
    L.check(lib.ivosw_jf_reduce_ragged(L.dptr(counts), L.int_array(n_obj), L.int_array(lengths), len(vids), metrics.METRIC_CODES[metric],
                                       L.dptr(annot) if state else None, L.dptr(per) if per_obj else None, L.dptr(quality),
                                       L.dptr(st) if state else None, L.stream_ptr(dev)), "jf_reduce_ragged")
    assert float(quality[rows]) == SENTINEL and (per is None or float(per[pairs]) == SENTINEL) and (st is None or bool((st[rows] == SENTINEL).all()))
    return (quality[:rows].cpu().numpy(), per[:pairs].cpu().numpy() if per_obj else None, st[:rows].cpu().numpy() if state else None,
            annot.cpu().numpy() if state else None)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("per_obj,state", [(False, False), (True, False), (False, True), (True, True)])
def test_reduce_equals_the_host_path_bit_for_bit(lib, dev, hand_counts, metric, per_obj, state):
    vids, want = hand_counts
    quality, per, st, annot = _reduce(lib, dev, vids, metric, per_obj, state)
    wq = np.concatenate(want[(metric, True)])
    np.testing.assert_array_equal(quality.view(np.int64), wq.view(np.int64))
    assert np.ptp(wq) > 0
    if per_obj:
        wp = np.concatenate([w.reshape(-1) for w in want[(metric, False)]])
        np.testing.assert_array_equal(per.view(np.int64), wp.view(np.int64))
    if state:
        np.testing.assert_array_equal(np.ascontiguousarray(st[:, 0]).view(np.uint32), wq.astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(st[:, 1], annot)


def test_reduce_128_sequences_of_ragged_lengths(lib, dev):
    vids = [R.make_counts(1 + (3 * k) % 5, R.OBJECT_COUNTS[k % len(R.OBJECT_COUNTS)], seed=100 + k) for k in range(L.MAX_SEQS)]
    assert min(c.shape[0] for c in vids) == 1
    quality, per, _, _ = _reduce(lib, dev, vids, "J_AND_F", True, False)
    wq = np.concatenate([R.host_metric(c, "J_AND_F", True) for c in vids])
    wp = np.concatenate([R.host_metric(c, "J_AND_F", False).reshape(-1) for c in vids])
    np.testing.assert_array_equal(quality.view(np.int64), wq.view(np.int64))
    np.testing.assert_array_equal(per.view(np.int64), wp.view(np.int64))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(lib, dev):
    rng = np.random.default_rng(5)
    a, b = _Vid(dev, rng, 2, 9, 20, [1, 2]), _Vid(dev, rng, 1, 6, 40, [3])
    msg = lambda: lib.ivosw_last_error().decode()
    total = (a.n * 2 + b.n) * 6
    counts = torch.full((total,), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    st = L.stream_ptr(dev)

    def call(descs, n=None, c=counts, w=ws, nbytes=None):
        table = (L.JfVideo * len(descs))(*descs)
        return lib.ivosw_jf_counts_videos(table, len(descs) if n is None else n, L.dptr(c) if c is not None else None,
                                          L.dptr(w) if w is not None else None, w.numel() if nbytes is None and w is not None else (nbytes or 0), st)

    def bad(v, **kw):
        d = v.desc()
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    for kw, text in ((dict(gt=None), "NULL"), (dict(pred=None), "NULL"), (dict(n_frames=0), "positive"), (dict(H=0), "positive"),
                     (dict(W=0), "positive"), (dict(n_obj=0), "1..32"), (dict(n_obj=33), "1..32"), (dict(bound_pix=-1), "0..32"),
                     (dict(bound_pix=33), "0..32"), (dict(n_frames=65535), "frames in total"), (dict(n_frames=30000, n_obj=3), "pairs in total")):
        assert call([a.desc(), bad(b, **kw)]) == -1 and "video 1:" in msg() and text in msg(), (kw, msg())
    assert call([a.desc(), b.desc()], n=0) == -1 and "n_videos 0" in msg()
    assert call([a.desc()] * (L.MAX_JF_VIDEOS + 1)) == -1 and "n_videos 33" in msg()
    assert call([a.desc(), b.desc()], c=None) == -1 and call([a.desc(), b.desc()], w=None) == -1 and "null pointer" in msg()
    assert call([a.desc(), b.desc()], nbytes=64) == -2 and "workspace 64 <" in msg()
    torch.cuda.synchronize(dev)
    assert bool((counts == SENTINEL).all())

    # the reduce entry: outputs pre-filled with a sentinel stay untouched
    cnts = torch.from_numpy(R.make_counts(6, 3, 1).reshape(-1)).to(dev)
    quality = torch.full((6,), float(SENTINEL), dtype=torch.float64, device=dev)
    per = torch.full((18,), float(SENTINEL), dtype=torch.float64, device=dev)
    state = torch.full((6, 2), float(SENTINEL), dtype=torch.float32, device=dev)
    annot = torch.zeros(6, dtype=torch.float32, device=dev)
    base = dict(counts=L.dptr(cnts), n_obj=L.int_array([3, 3]), lengths=L.int_array([4, 2]), n_seqs=2, metric=2, annot=L.dptr(annot), per=L.dptr(per),
                quality=L.dptr(quality), state=L.dptr(state))
    for kw, text in ((dict(counts=None), "null pointer"), (dict(n_obj=None), "null pointer"), (dict(lengths=None), "null pointer"),
                     (dict(quality=None), "null pointer"), (dict(state=None), "go together"), (dict(annot=None), "go together"),
                     (dict(metric=3), "unknown metric 3"), (dict(n_seqs=0), "n_seqs 0"), (dict(n_seqs=L.MAX_SEQS + 1), "n_seqs 129"),
                     (dict(lengths=L.int_array([4, 0])), "sequence 1"), (dict(lengths=L.int_array([-1, 2])), "sequence 0"),
                     (dict(n_obj=L.int_array([3, 0])), "video 1: n_obj 0"), (dict(n_obj=L.int_array([33, 3])), "video 0: n_obj 33")):
        args = dict(base, **kw)
        rc = lib.ivosw_jf_reduce_ragged(args["counts"], args["n_obj"], args["lengths"], args["n_seqs"], args["metric"], args["annot"], args["per"],
                                        args["quality"], args["state"], st)
        assert rc == -1 and text in msg(), (kw, msg())
    torch.cuda.synchronize(dev)
    assert bool((quality == SENTINEL).all()) and bool((per == SENTINEL).all()) and bool((state == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- the Python chain
def _sessions(dev, seed, shapes, on_device=True):
    rng = np.random.default_rng(seed)
    out = []
    for n, H, W, O in shapes:
        gt, pred = _labels(rng, n, H, W, O, range(1, O + 1))
        if on_device:
            gt, pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        out.append((gt, pred, O))
    return out


SHAPES = [(6, 24, 36, 2), (4, 31, 27, 1), (9, 18, 40, 9), (1, 7, 5, 3), (12, 40, 33, 3)]


def test_sequence_metric_videos_equals_sequence_metric(dev, monkeypatch):
    vids = _sessions(dev, 7, SHAPES[:3]) + _sessions(dev, 8, SHAPES[3:], on_device=False)       # device tensors and numpy arrays
    for metric in R.METRICS:
        for average in (True, False):
            want = [misc.sequence_metric(metric, g, p, o, average_over_objects=average) for g, p, o in vids]
            calls = []
            real_cpu = torch.Tensor.cpu
            monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
            got = misc.sequence_metric_videos(metric, vids, average_over_objects=average)
            monkeypatch.undo()
            assert calls == ["cpu"]                                       # ONE device-to-host copy
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == np.float64 and g.shape == w.shape
                np.testing.assert_array_equal(g.view(np.int64), np.ascontiguousarray(w).view(np.int64), err_msg=f"{metric} {average}")
            assert np.ptp(np.concatenate([w.reshape(-1) for w in want])) > 0


def _agent(dev, phase, candidates, skip, gap):
    cfg = AD(phase=phase, data=AD(subset="val"),
             agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500, update_rate=0.05, lr=5e-6, weight_decay=5e-4,
                      candidates=candidates, skip_annotated=skip, candidate_gap=gap))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    return agent


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("phase,seed,candidates,skip,gap", [("eval", 3, 1, False, 1), ("train", 2, 1, False, 1), ("eval", 3, 4, True, 1),
                                                            ("train", 2, 4, False, 3)])
def test_oracle_recommend_equals_the_per_session_path(dev, monkeypatch, capsys, K, phase, seed, candidates, skip, gap):
    agent = _agent(dev, phase, candidates, skip, gap)
    assert (agent.candidates, agent.skip_annotated, agent.candidate_gap) == (candidates, skip, gap)
    twin = copy.deepcopy(agent)
    vids = _sessions(dev, 11, SHAPES[:K])
    annotated = [[1, 1, 0], [0], [2, 5, 5, 8], [0, 0], [3, 4]][:K]
    cy = AD(setting="oracle", method="ours", davis_interactive=AD(metric="J_AND_F"), agent=AD(candidates=candidates, skip_annotated=skip,
                                                                                            candidate_gap=gap))
    sessions = [dict(gt_masks=g, pred_masks=p, n_objects=o, annotated_frames_list=list(a), prev_frames=sorted(set(a)))
                for (g, p, o), a in zip(vids, annotated)]
    for as_list in (False, True):
        random.seed(seed)
        np.random.seed(seed)
        want_m, want_p = [], []
        for s in sessions:
            m = misc.sequence_metric("J_AND_F", s["gt_masks"], s["pred_masks"], s["n_objects"])
            req = dict(n_frame=len(m), n_objects=s["n_objects"], all_F=None, all_P=None, new_masks_quality=m, prev_frames=s["prev_frames"],
                       annotated_frames_list=list(s["annotated_frames_list"]), mask_quality=None, first_frame=0, max_nb_interactions=8)
            want_m.append(m)
            want_p.append(utils_agent.recommend_candidates(cy, None, twin, dev, [req])[0] if as_list else
                          utils_agent.recommend_frame(cy, None, twin, dev, **req))
        log_want = capsys.readouterr().out
        rng_want = (random.random(), float(np.random.rand()))
        random.seed(seed)
        np.random.seed(seed)
        calls = []
        real_cpu, real_item, real_fwd, real_ragged = torch.Tensor.cpu, torch.Tensor.item, Brain.forward, Brain.forward_ragged
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
        monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item") if self.is_cuda else None, real_item(self))[1])
        monkeypatch.setattr(Brain, "forward", lambda self, *a, **k: (calls.append("forward"), real_fwd(self, *a, **k))[1])
        monkeypatch.setattr(Brain, "forward_ragged", lambda self, *a, **k: (calls.append("forward_ragged"), real_ragged(self, *a, **k))[1])
        got_m, got_p = utils_agent.oracle_recommend(cy, agent, dev, sessions, as_list=as_list)
        monkeypatch.undo()
        assert calls.count("cpu") == 1 and "item" not in calls, calls       # exactly ONE device-to-host copy
        assert [c for c in calls if c != "cpu"] in ([], ["forward"] if K == 1 else ["forward_ragged"]), calls
        assert capsys.readouterr().out == log_want
        for g, w in zip(got_m, want_m):
            assert g.dtype == np.float64
            np.testing.assert_array_equal(g.view(np.int64), w.view(np.int64))
            assert np.ptp(w) > 0 or len(w) == 1
        for g, w, s in zip(got_p, want_p, sessions):
            if as_list:
                np.testing.assert_array_equal(np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
                assert 1 <= len(g) <= candidates
            else:
                assert int(g) == int(w) and 0 <= int(g) < s["gt_masks"].shape[0]
        assert agent.steps_done == twin.steps_done
        assert (random.random(), float(np.random.rand())) == rng_want       # the host RNG streams moved as under sequential calls
    assert agent.steps_done == 2 * K


def test_oracle_recommend_worst_takes_the_quality_of_the_same_pass(dev, monkeypatch):
    vids = _sessions(dev, 13, SHAPES[:3])
    cy = AD(setting="oracle", method="worst", davis_interactive=AD(metric="J"), agent=AD(candidates=3, skip_annotated=False, candidate_gap=2))
    sessions = [dict(gt_masks=g, pred_masks=p, n_objects=o, annotated_frames_list=[0], prev_frames=pf) for (g, p, o), pf in zip(vids, ([0], None, [1, 2]))]
    for as_list in (False, True):
        want_m = [misc.sequence_metric("J", g, p, o) for g, p, o in vids]
        want_p = [(utils_agent.worst_candidates(m, 3, s["prev_frames"], 2) if as_list else
                   utils_agent.select_next_frame(m, metric="worst", prev_frames=s["prev_frames"])) for m, s in zip(want_m, sessions)]
        calls = []
        real_cpu = torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
        got_m, got_p = utils_agent.oracle_recommend(cy, None, dev, sessions, as_list=as_list)
        monkeypatch.undo()
        assert calls == ["cpu"]
        for g, w in zip(got_m, want_m):
            np.testing.assert_array_equal(g.view(np.int64), w.view(np.int64))
        for g, w in zip(got_p, want_p):
            np.testing.assert_array_equal(np.asarray(g), np.asarray(w))


# ---------------------------------------------------------------------------------------------- groups
def _many(dev, seed, n_videos, n_frames, H, W, O):
    """n_videos videos of one size as slices of ONE upload; and the same frames as one long video, which the host path scores at once."""
    rng = np.random.default_rng(seed)
    gt = torch.from_numpy(rng.integers(0, O + 1, (n_videos * n_frames, H, W)).astype(np.uint8)).to(dev)
    pred = torch.from_numpy(rng.integers(0, O + 1, (n_videos * n_frames, H, W)).astype(np.uint8)).to(dev)
    vids = [(gt[k * n_frames:(k + 1) * n_frames], pred[k * n_frames:(k + 1) * n_frames], O) for k in range(n_videos)]
    return vids, gt, pred


def _host_in_chunks(gt, pred, O, chunk):
    """sequence_metric of the long video, in chunks that fit the single-video entry's grid (frames are scored independently)."""
    return np.concatenate([misc.sequence_metric("J_AND_F", gt[a:a + chunk], pred[a:a + chunk], O) for a in range(0, gt.shape[0], chunk)])


def test_more_videos_than_the_table_holds(dev):
    vids, gt, pred = _many(dev, 17, 2 * L.MAX_JF_VIDEOS + 6, 1, 3, 5, 2)
    got = misc.sequence_metric_videos("J_AND_F", vids)
    want = _host_in_chunks(gt, pred, 2, 64)
    assert len(got) == len(vids) and all(g.shape == (1,) for g in got)
    np.testing.assert_array_equal(np.concatenate(got).view(np.int64), want.view(np.int64))
    assert np.ptp(want) > 0


@pytest.mark.parametrize("n_videos,n_frames,O,what", [(21, 100, 32, "pairs"), (32, 2100, 1, "frames")])
def test_a_group_beyond_a_flat_grid_dimension_is_split(lib, dev, n_videos, n_frames, O, what):
    vids, gt, pred = _many(dev, 19, n_videos, n_frames, 2, 3, O)
    groups = metrics._jf_groups([(n_frames, O)] * n_videos)
    assert len(groups) == 2 and n_videos <= L.MAX_JF_VIDEOS                # the grid limit splits the group, not the table size
    table = (L.JfVideo * n_videos)(*[L.JfVideo(gt=g.data_ptr(), pred=p.data_ptr(), n_frames=n_frames, H=2, W=3, n_obj=O, bound_pix=1)
                                     for g, p, _ in vids])
    assert lib.ivosw_jf_videos_ws_bytes(table, n_videos) == 0 and f"{what} in total" in lib.ivosw_last_error().decode()
    res = metrics.jf_videos(vids, "J_AND_F")
    got = res.quality.cpu().numpy()
    want = _host_in_chunks(gt, pred, O, 65535 // O // n_frames * n_frames or n_frames)
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
    assert [int(v.shape[0]) for v in res.views] == [n_frames] * n_videos and np.ptp(want) > 0


# ---------------------------------------------------------------------------------------------- the config key, end to end
@pytest.mark.parametrize("method", ["ours", "worst"])
def test_run_eval_oracle_is_the_same_under_metric_device(dev, tmp_path, monkeypatch, capsys, method):
    import re
    from ivos_w_amd import entry
    seen = {}
    for mode in ("host", "device"):
        cfg = entry.parse_cli(["with", "synthetic=1", "setting=oracle", f"method={method}", f"metric={mode}", "synth.n_sequences=2",
                               "synth.n_frames=8", "synth.height=48", "synth.width=80", "eval_max_nb_interactions=4", "agent.candidates=2",
                               f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/{mode}"])
        calls = []
        real = utils_agent.oracle_recommend
        monkeypatch.setattr(utils_agent, "oracle_recommend", lambda *a, **k: (calls.append(len(a[3])), real(*a, **k))[1])
        out = entry.run_eval(cfg, "MANet")
        monkeypatch.undo()
        lines = [re.sub(r"rec_time:\S+ ms", "", l) for l in capsys.readouterr().out.splitlines() if l.startswith("avg_")]
        assert (len(calls) == len(lines) and set(calls) == {1}) if mode == "device" else not calls
        assert len(lines) >= 8 and "candidates: [" in lines[0]
        seen[mode] = (out["auc"], out["curve"], lines)
    assert seen["host"] == seen["device"]
