"""ivosw_brain_topk_spread_ragged (the top-k with its k frames at least agent.candidate_gap apart) on the GPU: exact integer equality with
the numpy restatement of the greedy rule in tests/test_spread_option.py, `qv` bit-equal to q[idx], bit-equality with
ivosw_brain_topk_ragged at gap = 1, and the recommendation chain that ends in it (utils_agent.recommend_candidates, Agent.actions)."""
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.utils import utils_agent
from tests.test_gpu_topk import _Vid, _agent, _requests, assess, dev  # noqa: F401  (assess, dev: fixtures)
from tests.test_spread_option import spread_frames, spread_reference, spread_refusals
from tests.test_topk_option import AD, rank_frames

pytestmark = pytest.mark.gpu

# one trip of the wave, the edges of one trip, 256 / 257: the last length whose keys stay in registers (suppressed keys are zeroed there)
# and the first that is rebuilt from memory every round (tested against the accepted frames); 300: several trips of that path
LENGTHS = [1, 63, 64, 65, 256, 257, 300]
KS = [1, 4, 16]


def _state(counts, R, dev):
    st = np.stack([np.full(R, 0.5, dtype=np.float32), np.asarray(counts, dtype=np.float32)], 1)
    return torch.from_numpy(st).to(dev)


def _spread(dev, q, counts, lengths, k, skip, gap, first=None, plain=False):
    """The C entry on host arrays (`plain`: ivosw_brain_topk_ragged): (idx [K, k], qv [K, k]) with one guard row behind each checked."""
    K, R = len(lengths), sum(lengths)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    sd = _state(counts, R, dev) if counts is not None else None
    idx = torch.full((K + 1, k), -7, dtype=torch.int64, device=dev)
    qv = torch.full((K + 1, k), -7.5, dtype=torch.float32, device=dev)
    head = (L.dptr(qd), L.dptr(sd) if sd is not None else None, L.int_array(lengths), K, k, int(skip))
    tail = (L.dptr(idx), L.dptr(qv), L.stream_ptr(dev))
    if plain:
        L.check(L.lib().ivosw_brain_topk_ragged(*head, *tail), "topk_ragged")
    else:
        L.check(L.lib().ivosw_brain_topk_spread_ragged(*head, gap, L.int_array(first) if first is not None else None, *tail), "topk_spread_ragged")
    idx, qv = idx.cpu().numpy(), qv.cpu().numpy()
    assert (idx[K] == -7).all() and (qv[K] == -7.5).all()
    return idx[:K], qv[:K]


def _check(dev, q, counts, lengths, k, skip, gap, first=None):
    q = np.asarray(q, dtype=np.float32)
    idx, qv = _spread(dev, q, counts, lengths, k, skip, gap, first)
    want_idx, want_qv = spread_reference(q, counts, lengths, k, skip, gap, first)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(qv.view(np.int32), want_qv.view(np.int32))       # the bits of q[idx]; +0.0f at a -1 slot
    return idx


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)])


def _mixed(lengths, seed):
    """(q, counts): few values (many ties), with -0 / +0, both infinities and NaNs of either sign sprinkled in."""
    rs = np.random.RandomState(seed)
    R = sum(lengths)
    q = (rs.randint(-3, 4, R) / 2).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)
    where = rs.rand(R) < 0.15
    q[where] = special[rs.randint(0, len(special), int(where.sum()))]
    return q, (rs.rand(R) < 0.4).astype(np.float32)


@pytest.fixture(scope="module")
def mixed():
    return _mixed(LENGTHS, 7)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("k", KS)
def test_gap_1_without_a_forced_frame_is_the_plain_entry_bit_for_bit(dev, mixed, k, skip):
    q, counts = mixed
    idx, qv = _spread(dev, q, counts, LENGTHS, k, skip, 1)
    ref_idx, ref_qv = _spread(dev, q, counts, LENGTHS, k, skip, 1, plain=True)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(qv.view(np.int32), ref_qv.view(np.int32))
    _check(dev, q, counts, LENGTHS, k, skip, 1)
    if not skip:                                                        # no state at all with the flag clear
        np.testing.assert_array_equal(_spread(dev, q, None, LENGTHS, k, False, 1)[0], ref_idx)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("k", KS)
def test_gaps_equal_the_restated_rule(dev, mixed, k, skip):
    q, counts = mixed
    for gap in (2, 3, 7):
        idx = _check(dev, q, counts, LENGTHS, k, skip, gap)
        for row in idx:
            got = row[row >= 0]
            assert len(got) >= 1 and all(abs(int(x) - int(y)) >= gap for i, x in enumerate(got) for y in got[:i])
    for o, T in zip(_offsets(LENGTHS)[:-1], LENGTHS):                   # gap = T and T + 5: the first frame of the walk and nothing else
        for gap in (T, T + 5):
            idx = _check(dev, q[o:o + T], counts[o:o + T], [T], k, skip, gap)
            assert idx[0, 0] >= 0 and (idx[0, 1:] == -1).all()


@pytest.mark.parametrize("T", [5, 64, 256, 257, 300])
def test_constant_q_a_single_peak_and_exhaustion(dev, T):
    for k in KS:
        for gap in (2, 3, 7, T):
            idx = _check(dev, np.full(T, 0.25), None, [T], k, False, gap)
            want = list(range(0, T, gap))[:k]
            assert idx[0].tolist() == want + [-1] * (k - len(want))     # 0, g, 2g, ... then -1
    peak = T // 2
    q = -np.abs(np.arange(T) - peak).astype(np.float32)                 # one sharp peak, falling off on both sides
    for gap in (3, 7):
        idx = _check(dev, q, None, [T], 4, False, gap)
        got = idx[0][idx[0] >= 0]
        assert got[0] == peak and all(abs(int(t) - peak) >= gap for t in got[1:])
        if T > 2 * gap:
            assert sorted(got[1:3].tolist()) == [peak - gap, peak + gap]
    if T == 5:                                                          # exhaustion: two frames, two -1, qv 0.0 there
        idx, qv = _spread(dev, [1, 5, 2, 4, 3], None, [5], 4, False, 3)
        assert idx.tolist() == [[1, 4, -1, -1]] and qv.tolist() == [[5, 3, 0, 0]] and not np.signbit(qv[0, 2:]).any()


@pytest.mark.parametrize("T", [40, 300])
def test_tiers_under_skip_annotated(dev, T):
    q = np.linspace(1, 0, T).astype(np.float32)                          # falling: the walk is 0, 1, 2, ... inside a tier
    counts = np.zeros(T, dtype=np.float32)
    counts[8:] = 1                                                      # only frames 0 .. 7 are not annotated
    q[T - 1] = 9.0                                                      # the strongest frame of all is annotated and far away
    idx = _check(dev, q, counts, [T], 4, True, 5)
    # 1 .. 4 lie within the gap of 0 and are skipped, 5 is taken, 6 and 7 are skipped; only then the annotated tier: its best frame first
    assert idx[0].tolist() == [0, 5, T - 1, 10]
    idx = _check(dev, q, counts, [T], 4, False, 5)
    assert idx[0].tolist() == [T - 1, 0, 5, 10]                         # one tier without the flag
    counts[:] = 2                                                       # every frame annotated: falls through, the same rule
    idx = _check(dev, q, counts, [T], 3, True, 5)
    assert idx[0].tolist() == [T - 1, 0, 5]
    counts[:] = 0
    counts[3] = 1                                                       # an annotated frame suppresses nothing by itself
    idx = _check(dev, q[:20], counts[:20], [20], 4, True, 2)
    assert idx[0].tolist() == [0, 2, 4, 6]


@pytest.mark.parametrize("T", [40, 257])
def test_forced_first_candidate(dev, T):
    rs = np.random.RandomState(T)
    q = rs.randn(T).astype(np.float32)
    counts = (rs.rand(T) < 0.3).astype(np.float32)
    nan_at, annotated_at = T // 3, T // 2 + 1
    q[nan_at] = np.nan
    counts[annotated_at] = 3
    q[annotated_at] = -20.0                                             # the weakest frame of the weaker tier
    for first in (0, T - 1, T // 2, annotated_at, nan_at):
        for k in KS:
            for skip in (False, True):
                for gap in (1, 4):
                    idx = _check(dev, q, counts, [T], k, skip, gap, [first])
                    got = idx[0][idx[0] >= 0]
                    assert got[0] == first and all(abs(int(t) - first) >= gap for t in got[1:]) and first not in got[1:]
    idx, qv = _spread(dev, q, counts, [T], 2, True, 4, [nan_at])
    assert idx[0, 0] == nan_at and np.isnan(qv[0, 0]) and not np.isnan(qv[0, 1])
    _check(dev, q, counts, [T], 4, True, T, [T // 2])                   # the forced frame alone


@pytest.mark.parametrize("n_seqs", [1, 3, 128])
def test_sessions_equal_the_kernel_on_each_alone(dev, n_seqs):
    rs = np.random.RandomState(n_seqs)
    lengths = {1: [65], 3: [257, 1, 100], 128: [1 + (37 * s) % 90 for s in range(127)] + [300]}[n_seqs]
    q, counts = _mixed(lengths, 100 + n_seqs)
    first = [int(rs.randint(-1, n)) if s % 3 else -1 for s, n in enumerate(lengths)]      # mixed: some forced, some not
    k, gap = 4, 3
    idx, qv = _spread(dev, q, counts, lengths, k, True, gap, first)
    want_idx, want_qv = spread_reference(q, counts, lengths, k, True, gap, first)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(qv.view(np.int32), want_qv.view(np.int32))
    for s, (o, n) in enumerate(zip(_offsets(lengths)[:-1], lengths)):
        alone_idx, alone_qv = _spread(dev, q[o:o + n], counts[o:o + n], [n], k, True, gap, [first[s]])
        np.testing.assert_array_equal(alone_idx[0], idx[s])
        np.testing.assert_array_equal(alone_qv[0].view(np.int32), qv[s].view(np.int32))


def test_refusals_name_the_argument_and_leave_idx_untouched(dev):
    q = torch.zeros(8, device=dev)
    state = torch.zeros(8, 2, device=dev)
    idx = torch.full((2, 16), -7, dtype=torch.int64, device=dev)
    qv = torch.full((2, 16), -7.5, dtype=torch.float32, device=dev)
    res = spread_refusals(L.lib(), L.dptr(q), L.dptr(state), L.dptr(idx), L.dptr(qv))
    assert len(res) == 18
    for rc, message, words in res:
        assert rc == -1 and all(w in message for w in words), (message, words)
    torch.cuda.synchronize(dev)
    assert bool((idx == -7).all()) and bool((qv == -7.5).all())


# ---------------------------------------------------------------------------------------------- the recommendation chain
@pytest.fixture(scope="module")
def long_videos(dev):
    g = torch.Generator().manual_seed(5)
    return [_Vid(dev, g, 21, 1), _Vid(dev, g, 17, 2)]


def _restated(agent, req, k, skip, gap):
    counts = utils_agent._annotation_counts(req["n_frame"], req["annotated_frames_list"])
    state = np.stack([req["mask_quality"].astype(np.float32), counts.astype(np.float32)], 1)
    q = agent.policy_net(torch.from_numpy(state).to(agent.device)[None])[0].cpu().numpy()
    return spread_frames(rank_frames(q, counts, skip), k, gap)


@pytest.mark.parametrize("method", ["ours", "worst"])
def test_recommend_candidates_are_spread(dev, assess, long_videos, method):
    annotated = [[3, 3, 12], [8]]
    k, gap = 4, 5
    cy = AD(setting="wild", method=method, agent=AD(candidates=k, skip_annotated=True, candidate_gap=gap))
    plain_cy = AD(setting="wild", method=method, agent=AD(candidates=k, skip_annotated=True))
    agent = _agent(dev, candidates=k, skip_annotated=True, candidate_gap=gap) if method == "ours" else None
    plain = _agent(dev, candidates=k, skip_annotated=True) if method == "ours" else None
    want_req = _requests(long_videos, annotated)
    dense = utils_agent.recommend_candidates(plain_cy, assess, plain, dev, want_req)
    got_req = _requests(long_videos, annotated)
    got = utils_agent.recommend_candidates(cy, assess, agent, dev, got_req)
    firsts = utils_agent.recommend_frames(cy, assess, agent, dev, _requests(long_videos, annotated))
    for c, d, f, a, b, v in zip(got, dense, firsts, got_req, want_req, long_videos):
        np.testing.assert_array_equal(a["mask_quality"].view(np.int64), b["mask_quality"].view(np.int64))        # filled as before
        assert np.ptp(a["mask_quality"]) > 0
        assert isinstance(c, np.ndarray) and c.dtype == np.int64 and 1 <= len(c) <= k and all(0 <= int(t) < v.n for t in c)
        assert all(abs(int(x) - int(y)) >= gap for i, x in enumerate(c) for y in c[:i])
        assert int(c[0]) == int(f) == int(d[0])                         # candidate 0 is what a gap never changes
        if method == "ours":
            assert c.tolist() == _restated(agent, a, k, True, gap).tolist()
        else:
            assert c.tolist() == utils_agent.worst_candidates(a["mask_quality"], k, a["prev_frames"], gap).tolist()
            order = [int(t) for t in np.argsort(a["mask_quality"], kind="stable")]
            prev = a["prev_frames"]
            order = [t for t in order if t not in prev] + [t for t in order if t in prev]
            assert c.tolist() == spread_frames(order, k, gap).tolist()
    # the single-request chain (Brain.forward and a one-sequence launch): the same lists
    utils_agent.clear_frame_cache()
    for v, a, c in zip(long_videos, annotated, got):
        single = utils_agent.recommend_candidates(cy, assess, agent, dev, _requests([v], [a]))
        assert len(single) == 1 and single[0].tolist() == c.tolist()
    utils_agent.clear_frame_cache()


def test_actions_on_the_epsilon_branch_put_the_pick_first(dev, capsys):
    k, gap = 4, 3
    agent, plain = _agent(dev, phase="train", candidates=k, candidate_gap=gap), _agent(dev, phase="train", candidates=k)
    rs = np.random.RandomState(11)
    states = [np.stack([rs.rand(n), rs.randint(0, 2, n).astype(np.float64)], 1).astype(np.float32) for n in (30, 12, 70)]
    random.seed(2)
    ref = plain.actions(states)
    log_ref = capsys.readouterr().out
    random.seed(2)
    got = agent.actions(states)
    assert capsys.readouterr().out == log_ref and agent.steps_done == plain.steps_done == 3
    randomly = ["randomly" in ln for ln in log_ref.splitlines()]
    assert 0 < sum(randomly) < 3, randomly                               # (the seed gives both branches)
    for s, r, g, rnd in zip(states, ref, got, randomly):
        q = agent.policy_net(torch.from_numpy(s).to(dev)[None])[0].cpu().numpy()
        pick = int(r[0]) if rnd else -1
        assert g.tolist() == spread_frames(rank_frames(q), k, gap, pick).tolist()
        assert all(abs(int(x) - int(y)) >= gap for i, x in enumerate(g) for y in g[:i])
        assert int(g[0]) == (pick if rnd else int(np.argmax(q)))
    out = torch.full((3, k), -7, dtype=torch.int64, device=dev)         # device_out: the ranking is left there complete
    random.seed(2)
    picks = agent.actions(states, verbose=False, device_out=out)
    assert [p is not None for p in picks] == randomly
    assert [row[row >= 0].tolist() for row in out.cpu().numpy()] == [g.tolist() for g in got]
