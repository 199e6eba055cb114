"""agent.candidate_gap and ivosw_brain_topk_spread_ragged, the parts that need no GPU: a numpy restatement of the greedy rule
(``spread_reference``, which the GPU tests compare against exactly), its agreement with ``worst_candidates`` on the "worst" order, option
validation, the CLI key, the host half of Agent.action / Agent.actions under a gap (steps_done, the two host RNG streams, the log), and
that nothing new is entered at candidate_gap = 1."""
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models import agent as agent_mod
from ivos_w_amd.models.agent import Agent, Brain, candidate_gap_option, spread_candidates
from ivos_w_amd.utils import utils_agent
from tests.test_topk_option import AD, _cfg, rank_frames


# ---------------------------------------------------------------------------------------------- the rule, restated in numpy
def spread_frames(order, k, gap, first=-1):
    """The greedy walk over ONE sequence's frames in `order` (the strongest first): a frame is accepted if and only if it lies `gap` or
    more frames from every accepted one, until k are accepted.  `first` >= 0 is accepted before the walk, as slot 0."""
    taken = [int(first)] if first >= 0 else []
    for t in order:
        if len(taken) >= k:
            break
        if all(abs(int(t) - w) >= gap for w in taken):
            taken.append(int(t))
    return np.array(taken[:k], dtype=np.int64)


def spread_reference(q, counts, lengths, k, skip, gap, first=None):
    """(idx int64 [K, k], qv float32 [K, k]) of ivosw_brain_topk_spread_ragged over the flat q / counts: the order of
    ivosw_brain_topk_ragged (tests/test_topk_option.py's rank_frames) walked greedily; -1 and 0.0f from the slot on at which nothing more
    can be accepted."""
    q = np.asarray(q, dtype=np.float32)
    idx = np.full((len(lengths), k), -1, dtype=np.int64)
    qv = np.zeros((len(lengths), k), dtype=np.float32)
    off = 0
    for s, n in enumerate(lengths):
        order = rank_frames(q[off:off + n], None if counts is None else np.asarray(counts)[off:off + n], skip)
        got = spread_frames(order, k, gap, -1 if first is None else first[s])
        idx[s, :len(got)] = got
        qv[s, :len(got)] = q[off:off + n][got]
        off += n
    return idx, qv


def test_the_restated_rule_on_small_cases():
    order = rank_frames([1, 9, 8, 7, 2, 6])                                               # 1 2 3 5 4 0
    assert spread_frames(order, 3, 1).tolist() == [1, 2, 3]                               # gap 1: the ranking itself
    assert spread_frames(order, 3, 2).tolist() == [1, 3, 5]
    assert spread_frames(order, 3, 3).tolist() == [1, 5]                                  # 4 is within 3 of both: nothing comes back
    assert spread_frames(order, 3, 6).tolist() == [1]
    assert spread_frames(order, 3, 2, first=4).tolist() == [4, 1]                         # the forced frame suppresses 3 and 5; 1 suppresses 2, 0
    assert spread_frames(order, 1, 2, first=4).tolist() == [4]
    assert spread_frames(order, 4, 1, first=4).tolist() == [4, 1, 2, 3]                   # gap 1: the forced frame only suppresses itself
    idx, qv = spread_reference([0.5] * 5, None, [5], 4, False, 3)
    assert idx.tolist() == [[0, 3, -1, -1]] and qv.tolist() == [[0.5, 0.5, 0, 0]]         # constant q: 0, g, 2g .. then -1
    # tiers: an unannotated frame within the gap of an accepted one is skipped; the far annotated one comes after the tier is exhausted
    idx, _ = spread_reference([9, 8, 1, 1, 1, 7], [0, 0, 0, 1, 0, 1], [6], 4, True, 2)
    assert idx.tolist() == [[0, 2, 4, -1]]
    idx, _ = spread_reference([9, 8, 1, 7], [0, 0, 1, 1], [4], 3, True, 2)
    assert idx.tolist() == [[0, 3, -1]]                                                   # 1 is suppressed, 3 is annotated but all that is left
    idx, _ = spread_reference([1, 3, 2, 7, 5], None, [3, 2], 2, False, 2, first=[-1, 1])
    assert idx.tolist() == [[1, -1], [1, -1]]


@pytest.mark.parametrize("seed", range(8))
def test_worst_candidates_follow_the_restated_rule(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 40))
    v = rs.permutation(n).astype(np.float64) / n                                          # tie-free
    prev = [int(i) for i in rs.choice(n, size=int(rs.randint(0, n + 1)), replace=False)]  # from none to every frame annotated
    counts = utils_agent._annotation_counts(n, prev)
    for k in (1, 4, 16):
        for gap in (1, 2, 5, n, n + 3):
            want = spread_frames(rank_frames(-v, counts, skip=True), k, gap)
            assert utils_agent.worst_candidates(v, k, prev, gap).tolist() == want.tolist()
            want = spread_frames(rank_frames(-v), k, gap)
            assert utils_agent.worst_candidates(v, k, None, gap).tolist() == want.tolist()
        assert utils_agent.worst_candidates(v, k, prev, 1).tolist() == utils_agent.worst_candidates(v, k, prev).tolist()


def test_worst_candidates_through_recommend_candidates_read_the_key_from_the_config():
    q = np.array([0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.8])
    req = dict(n_frame=7, n_objects=1, all_F=None, all_P=None, new_masks_quality=q, prev_frames=[1], annotated_frames_list=[1],
               mask_quality=None, first_frame=1, max_nb_interactions=8)
    plain = AD(setting="oracle", method="worst", agent=AD(candidates=3))
    spread = AD(setting="oracle", method="worst", agent=AD(candidates=3, candidate_gap=2))
    assert [c.tolist() for c in utils_agent.recommend_candidates(plain, None, None, "cpu", [req, req])] == [[5, 3, 0]] * 2
    assert [c.tolist() for c in utils_agent.recommend_candidates(spread, None, None, "cpu", [req, req])] == [[5, 3, 0]] * 2
    spread.agent["candidate_gap"] = 3
    assert [c.tolist() for c in utils_agent.recommend_candidates(spread, None, None, "cpu", [req])] == [[5, 0]]      # 3, 4, 6, 2 fall inside
    assert [int(i) for i in utils_agent.recommend_frames(spread, None, None, "cpu", [req])] == [5]
    one = AD(setting="oracle", method="worst", agent=AD(candidates=1, candidate_gap=3))   # one candidate: a gap has no effect
    assert [c.tolist() for c in utils_agent.recommend_candidates(one, None, None, "cpu", [req])] == [[5]]
    with pytest.raises(ValueError, match=r"agent\.candidate_gap"):
        utils_agent.recommend_candidates(AD(setting="oracle", method="worst", agent=AD(candidates=3, candidate_gap=0)), None, None, "cpu", [req])


# ---------------------------------------------------------------------------------------------- options
def test_option_default_and_accepted_values():
    assert agent_mod.MAX_CANDIDATE_GAP == 1 << 20
    assert Agent("cpu", _cfg()).candidate_gap == 1                                        # a config without the key
    assert Agent("cpu", _cfg(candidate_gap=1)).candidate_gap == 1
    assert Agent("cpu", _cfg(candidates=4, candidate_gap=1 << 20)).candidate_gap == 1 << 20
    assert candidate_gap_option() == 1 and candidate_gap_option(7) == 7
    assert entry.DEFAULTS["agent"]["candidate_gap"] == 1


@pytest.mark.parametrize("bad", [0, -1, True, 1.5, "2", (1 << 20) + 1, None])
def test_a_bad_gap_is_refused_and_names_the_key(bad):
    with pytest.raises(ValueError, match=r"agent\.candidate_gap"):
        Agent("cpu", _cfg(candidate_gap=bad))
    with pytest.raises(ValueError, match=r"agent\.candidate_gap"):
        candidate_gap_option(bad)


def test_parse_cli_accepts_the_key():
    cfg = entry.parse_cli(["with", "agent.candidates=4", "agent.candidate_gap=5"])
    assert cfg.agent.candidate_gap == 5 and Agent("cpu", cfg).candidate_gap == 5
    assert entry.parse_cli([]).agent.candidate_gap == 1


def test_the_real_stack_still_refuses_several_candidates():
    cfg = entry.parse_cli(["agent.candidates=2", "agent.candidate_gap=3"])
    with pytest.raises(ValueError, match=r"agent\.candidates"):
        entry.run_eval_real(cfg, "MANet", torch.device("cpu"))


def test_spread_candidates_only_cuts_the_empty_slots():
    assert spread_candidates(np.array([7, 2, -1, -1])).tolist() == [7, 2]
    assert spread_candidates(np.array([3])).dtype == np.int64 and spread_candidates(np.array([-1, -1])).tolist() == []


# ---------------------------------------------------------------------------------------------- the C entry's refusals
@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def spread_refusals(lib, q, state, idx, qv):
    """Every refused call of the entry on the given (never dereferenced) pointers: [(return code, message, words the message must hold)]."""
    arr, none = L.int_array([3, 5]), None
    spread = lib.ivosw_brain_topk_spread_ragged
    msg = lambda: lib.ivosw_last_error().decode()
    calls = [((none, state, arr, 2, 1, 0, 2, none, idx, qv, none), ["q is a null pointer"]),
             ((q, state, none, 2, 1, 0, 2, none, idx, qv, none), ["lengths is a null pointer"]),
             ((q, state, arr, 2, 1, 0, 2, none, none, qv, none), ["idx is a null pointer"])]
    calls += [((q, state, arr, 2, k, 0, 2, none, idx, none, none), ["k ", str(k), "[1, 16]"]) for k in (0, 17, -3)]
    calls += [((q, none, arr, 2, 2, 1, 2, none, idx, none, none), ["skip_annotated", "state"]),
              ((q, none, arr, 0, 2, 0, 2, none, idx, none, none), ["n_seqs"]),
              ((q, none, arr, 129, 2, 0, 2, none, idx, none, none), ["n_seqs"]),
              ((q, state, L.int_array([3, 0]), 2, 2, 1, 2, none, idx, none, none), ["sequence 1"]),
              ((q, none, L.int_array([1 << 20, 1]), 2, 1, 0, 2, none, idx, none, none), ["2^20"])]
    calls += [((q, none, arr, 2, 2, 0, gap, none, idx, none, none), ["gap", str(gap)]) for gap in (0, -1, (1 << 20) + 1)]
    calls += [((q, none, arr, 2, 2, 0, 2, L.int_array(first), idx, none, none), [f"first[{s}]", str(first[s])])
              for s, first in ((0, [3, 0]), (1, [2, 5]), (1, [-1, -2]), (0, [-5, 9]))]
    out = []
    for args, words in calls:
        rc = spread(*args)
        out.append((rc, msg(), words + ["ivosw_brain_topk_spread_ragged"]))
    return out


def test_spread_entry_refusals_do_not_touch_the_gpu(lib):
    import ctypes
    fake = ctypes.c_void_p(0x10000)                                 # a made-up address: a refused call dereferences nothing
    res = spread_refusals(lib, fake, fake, fake, fake)
    assert len(res) == 18
    for rc, message, words in res:
        assert rc == -1 and all(w in message for w in words), (message, words)


# ---------------------------------------------------------------------------------------------- the host half under a gap
def _stand_in(agent, calls):
    """Replaces the device half: the order of a state is the rising order of its first column, spread by the rule when a gap is given."""
    def ranked(states, k=None, skip_annotated=None, out=None, gap=1, first=None):
        calls.append((len(states), gap, None if first is None else list(first)))
        rank = torch.full((len(states), k), -1, dtype=torch.int64)
        for i, s in enumerate(states):
            order = np.argsort(np.asarray(s.cpu() if torch.is_tensor(s) else s)[:, 0], kind="stable")
            got = spread_frames(order, k, gap, -1 if first is None else first[i])
            rank[i, :len(got)] = torch.from_numpy(got)
        if out is not None:
            out.view(len(states), k).copy_(rank)
            return out
        return rank
    agent.candidates_device = ranked
    agent.greedy_index_device = agent.greedy_indices_device = None          # the argmax path is not taken


@pytest.mark.parametrize("phase", ["train", "eval"])
def test_the_host_half_moves_alike_at_gap_3_and_gap_1(phase, capsys):
    rs = np.random.RandomState(5)
    states = [np.stack([rs.rand(n), rs.randint(0, 3, n).astype(np.float64)], 1) for n in (7, 12, 5, 9, 30, 2)]
    k = 4
    plain, a, b, c = (Agent("cpu", _cfg(phase, candidates=k, skip_annotated=True, candidate_gap=g)) for g in (1, 3, 3, 3))
    calls = {id(ag): [] for ag in (plain, a, b, c)}
    for ag in (plain, a, b, c):
        ag.steps_done = 40
        _stand_in(ag, calls[id(ag)])
    out = torch.full((6, k), -7, dtype=torch.int64)
    runs = []
    for run in (lambda: [plain.action(s) for s in states], lambda: [a.action(s) for s in states], lambda: b.actions(states),
                lambda: c.actions(states, device_out=out)):
        random.seed(2)
        np.random.seed(2)
        res = run()
        runs.append((res, capsys.readouterr().out, random.random(), float(np.random.rand())))
    (ref, log_ref, *rng_ref), (one, log_one, *rng_one), (many, log_many, *rng_many), (left, log_left, *rng_left) = runs
    assert log_ref == log_one == log_many == log_left and log_ref.count("step:") == 6
    assert rng_ref == rng_one == rng_many == rng_left                   # both host RNG streams end where gap = 1 leaves them
    assert plain.steps_done == a.steps_done == b.steps_done == c.steps_done == 46
    randomly = ["randomly" in ln for ln in log_ref.splitlines()]
    assert (0 < sum(randomly) < 6) if phase == "train" else not any(randomly)
    picks = [int(r[0]) if rnd else -1 for r, rnd in zip(ref, randomly)]                  # gap 1: the pick is merged in as entry 0
    # gap 1 calls the device half exactly as before (no gap, no first); gap 3 hands the picks on as the forced first candidates
    assert calls[id(plain)] == [(1, 1, None)] * 6
    assert calls[id(a)] == [(1, 3, [p]) for p in picks] and calls[id(b)] == [(6, 3, picks)] and calls[id(c)] == [(6, 3, picks)]
    assert left == [None if p < 0 else p for p in picks]                                  # device_out: None marks a greedy state
    for s, w, g, row, p in zip(states, one, many, out.numpy(), picks):
        want = spread_frames(np.argsort(s[:, 0], kind="stable"), k, 3, p)
        assert isinstance(g, np.ndarray) and g.dtype == np.int64
        assert g.tolist() == w.tolist() == want.tolist() == row[row >= 0].tolist()        # final as it comes: nothing is merged
        assert (row[len(want):] == -1).all()
        if p >= 0:
            assert int(g[0]) == p and all(abs(int(t) - p) >= 3 for t in g[1:])
        assert all(abs(int(x) - int(y)) >= 3 for i, x in enumerate(g) for y in g[:i])


def test_one_candidate_ignores_the_gap(capsys):
    a = Agent("cpu", _cfg("eval", candidates=1, skip_annotated=True, candidate_gap=9))
    calls = []
    _stand_in(a, calls)
    state = np.stack([np.array([3., 1., 2.]), np.zeros(3)], 1)
    got = a.action(state, verbose=False)
    assert isinstance(got, np.int64) and int(got) == 1 and calls == [(1, 1, None)]
    assert [int(v) for v in a.actions([state, state], verbose=False)] == [1, 1] and calls[-1] == (2, 1, None)


# ---------------------------------------------------------------------------------------------- gap = 1 enters nothing new
class _FakeLib:
    """Stands in for the library below Agent.topk_ragged: the plain entry fills idx with 0 .. k - 1, the spread entry is recorded (or
    refuses to be called at all)."""

    def __init__(self, forbid_spread):
        self.plain, self.spread, self.forbid = [], [], forbid_spread

    def ivosw_brain_topk_ragged(self, q, state, lengths, n_seqs, k, skip, idx, qv, stream):
        self.plain.append((n_seqs, k, skip))
        idx.copy_(torch.arange(k).expand(n_seqs, k))
        return 0

    def ivosw_brain_topk_spread_ragged(self, q, state, lengths, n_seqs, k, skip, gap, first, idx, qv, stream):
        if self.forbid:
            raise AssertionError("ivosw_brain_topk_spread_ragged was called at candidate_gap = 1")
        self.spread.append((n_seqs, k, skip, gap, None if first is None else list(first)))
        idx.copy_(torch.arange(k).expand(n_seqs, k) * gap)
        return 0


def _on_the_host(monkeypatch, fake):
    monkeypatch.setattr(L, "lib", lambda: fake)
    monkeypatch.setattr(L, "dptr", lambda t, dtype=None: t)
    monkeypatch.setattr(L, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(Brain, "forward", lambda self, x: torch.zeros(x.shape[0], x.shape[1]))
    monkeypatch.setattr(Brain, "forward_ragged", lambda self, x, lengths=None: (torch.zeros(x.shape[0]), None))


def test_gap_1_calls_the_plain_entry_and_never_the_new_binding(monkeypatch):
    fake = _FakeLib(forbid_spread=True)
    _on_the_host(monkeypatch, fake)
    states = [np.stack([np.linspace(0, 1, n), np.zeros(n)], 1) for n in (9, 12)]
    for options in (dict(candidates=3), dict(candidates=3, candidate_gap=1), dict(candidates=1, skip_annotated=True, candidate_gap=8)):
        a = Agent("cpu", _cfg("train", **options))
        a.EPS_START = a.EPS_END = 0.5                                   # both branches occur
        random.seed(3)
        for _ in range(4):
            a.action(states[0], verbose=False)
            a.actions(states, verbose=False)
            a.actions(states, verbose=False, device_out=torch.zeros(2, a.candidates, dtype=torch.int64))
        a.candidates_device(states)
        a.topk_ragged(torch.zeros(21), torch.zeros(21, 2), [9, 12], a.candidates, False)
    assert len(fake.plain) > 20 and fake.spread == []


def test_gap_3_calls_the_new_entry_with_the_picks(monkeypatch):
    fake = _FakeLib(forbid_spread=False)
    _on_the_host(monkeypatch, fake)
    states = [np.stack([np.linspace(0, 1, n), np.zeros(n)], 1) for n in (9, 12)]
    a = Agent("cpu", _cfg("train", candidates=3, candidate_gap=3))
    a.EPS_START = a.EPS_END = 2.0                                       # every draw is random
    random.seed(3)
    got = a.actions(states, verbose=False)
    (n_seqs, k, skip, gap, first), = fake.spread
    assert (n_seqs, k, skip, gap) == (2, 3, 0, 3) and all(0 <= f < n for f, n in zip(first, (9, 12))) and fake.plain == []
    assert [g.tolist() for g in got] == [[0, 3, 6]] * 2                 # what the entry wrote, as it stands
    a.EPS_START = a.EPS_END = 0.0                                       # greedy: no forced candidate
    assert a.action(states[1], verbose=False).tolist() == [0, 3, 6] and fake.spread[-1] == (1, 3, 0, 3, [-1])
    with pytest.raises(ValueError, match="forced first"):
        a.topk_ragged(torch.zeros(21), None, [9, 12], 3, False, gap=2, first=[1])
