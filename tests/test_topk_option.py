"""agent.candidates / agent.skip_annotated and ivosw_brain_topk_ragged, the parts that need no GPU: option validation, the CLI keys, the
C entry's refusals, the host half of Agent.action / Agent.actions with k > 1 (steps_done, the two host RNG streams, the epsilon-branch
merge), and a numpy restatement of the entry's total order (``topk_reference``), which the GPU tests compare against exactly."""
import ctypes
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models.agent import Agent, candidates_option, merge_candidates
from ivos_w_amd.utils import utils_agent


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


# ---------------------------------------------------------------------------------------------- the order, restated in numpy
def rank_frames(q, counts=None, skip=False):
    """All frames of ONE sequence, the strongest first, by the order of ivosw_brain_topk_ragged: the tier (not annotated before
    annotated, under `skip`), then the larger q (-0 == +0, NaN below every number), then the lower index."""
    q = np.asarray(q, dtype=np.float32)
    n = len(q)
    nan = np.isnan(q)
    value = np.where(nan, np.float32(0), q) + np.float32(0)             # (-0) + (+0) = +0
    tier = (np.asarray(counts) != 0) if skip else np.zeros(n, dtype=bool)
    return np.lexsort((np.arange(n), -value, nan, tier)).astype(np.int64)       # the last key is the primary one


def topk_reference(q, counts, lengths, k, skip):
    """(idx int64 [K, k], qv float32 [K, k]) of ivosw_brain_topk_ragged over the flat q / counts: -1 and 0.0f from a sequence's length on."""
    q = np.asarray(q, dtype=np.float32)
    idx = np.full((len(lengths), k), -1, dtype=np.int64)
    qv = np.zeros((len(lengths), k), dtype=np.float32)
    off = 0
    for s, n in enumerate(lengths):
        order = rank_frames(q[off:off + n], None if counts is None else np.asarray(counts)[off:off + n], skip)[:k]
        idx[s, :len(order)] = order
        qv[s, :len(order)] = q[off:off + n][order]
        off += n
    return idx, qv


def test_the_restated_order_on_small_cases():
    inf, nan = np.inf, np.nan
    assert rank_frames([1, 3, 2]).tolist() == [1, 2, 0]
    assert rank_frames([2, 2, 2]).tolist() == [0, 1, 2]                                   # equal values: rising index
    assert rank_frames([-0.0, 0.0, -1, 0.0]).tolist() == [0, 1, 3, 2]                     # -0 before +0 at equal rank
    assert rank_frames([nan, -inf, inf, 1]).tolist() == [2, 3, 1, 0]                      # NaN below -inf
    assert rank_frames([nan, nan]).tolist() == [0, 1]
    assert rank_frames([5, 4, 3], [1, 0, 0], skip=True).tolist() == [1, 2, 0]             # the annotated frame comes last
    assert rank_frames([5, 4, 3], [1, 0, 0], skip=False).tolist() == [0, 1, 2]
    assert rank_frames([5, 4, 3], [1, 2, 1], skip=True).tolist() == [0, 1, 2]             # all annotated: falls through
    assert rank_frames([nan, 1], [0, 1], skip=True).tolist() == [0, 1]                    # the tier outranks the value
    idx, qv = topk_reference([1, 3, 2, 7], None, [3, 1], 2, False)
    assert idx.tolist() == [[1, 2], [0, -1]] and qv.tolist() == [[3, 2], [7, 0]]


@pytest.mark.parametrize("seed", range(6))
def test_the_restated_order_agrees_with_select_next_frame(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 40))
    q = rs.permutation(n).astype(np.float64) - n / 3                                      # tie-free
    prev = [int(i) for i in rs.choice(n, size=int(rs.randint(0, n + 1)), replace=False)]  # from none to every frame annotated
    counts = utils_agent._annotation_counts(n, prev + prev[:2])
    assert int(rank_frames(q, counts, skip=True)[0]) == int(utils_agent.select_next_frame(q.copy(), "max", prev))
    assert int(rank_frames(q, counts, skip=False)[0]) == int(utils_agent.select_next_frame(q.copy(), "max", None)) == int(np.argmax(q))


# ---------------------------------------------------------------------------------------------- options
def _cfg(phase="eval", **agent):
    return AD(phase=phase, data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4, **agent))


def test_options_default_and_accepted_values():
    assert L.MAX_CANDIDATES == 16
    a = Agent("cpu", _cfg())
    assert (a.candidates, a.skip_annotated) == (1, False)
    a = Agent("cpu", _cfg(candidates=16, skip_annotated=True))
    assert (a.candidates, a.skip_annotated) == (16, True)
    assert candidates_option(4, False) == (4, False)
    assert entry.DEFAULTS["agent"]["candidates"] == 1 and entry.DEFAULTS["agent"]["skip_annotated"] is False


@pytest.mark.parametrize("bad", [0, 17, -1, 2.0, "3", True, None])
def test_bad_candidates_are_refused_and_name_the_key(bad):
    with pytest.raises(ValueError, match=r"agent\.candidates"):
        Agent("cpu", _cfg(candidates=bad))


@pytest.mark.parametrize("bad", [0, 1, "true", None, 0.0])
def test_bad_skip_annotated_is_refused_and_names_the_key(bad):
    with pytest.raises(ValueError, match=r"agent\.skip_annotated"):
        Agent("cpu", _cfg(skip_annotated=bad))


def test_parse_cli_accepts_the_keys():
    cfg = entry.parse_cli(["with", "agent.candidates=4", "agent.skip_annotated=true"])
    assert cfg.agent.candidates == 4 and cfg.agent.skip_annotated is True
    cfg = entry.parse_cli([])
    assert cfg.agent.candidates == 1 and cfg.agent.skip_annotated is False
    a = Agent("cpu", entry.parse_cli(["agent.candidates=3", "agent.skip_annotated=false"]))
    assert (a.candidates, a.skip_annotated) == (3, False)


def test_the_real_stack_refuses_several_candidates():
    cfg = entry.parse_cli(["agent.candidates=2"])
    with pytest.raises(ValueError, match=r"agent\.candidates"):
        entry.run_eval_real(cfg, "MANet", torch.device("cpu"))


# ---------------------------------------------------------------------------------------------- the C entry's refusals
@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_topk_entry_refusals_do_not_touch_the_gpu(lib):
    msg = lambda: lib.ivosw_last_error().decode()
    arr = L.int_array([3, 5])
    fake = ctypes.c_void_p(0x10000)                                 # a made-up address: a refused call dereferences nothing
    topk = lib.ivosw_brain_topk_ragged
    assert topk(None, fake, arr, 2, 1, 0, fake, fake, None) == -1 and "q is a null pointer" in msg()
    assert topk(fake, fake, None, 2, 1, 0, fake, fake, None) == -1 and "lengths is a null pointer" in msg()
    assert topk(fake, fake, arr, 2, 1, 0, None, fake, None) == -1 and "idx is a null pointer" in msg()
    for k in (0, 17, -3):
        assert topk(fake, fake, arr, 2, k, 0, fake, None, None) == -1 and "k " in msg() and str(k) in msg() and "[1, 16]" in msg()
    assert topk(fake, None, arr, 2, 2, 1, fake, None, None) == -1 and "skip_annotated" in msg() and "state" in msg()
    assert topk(fake, None, arr, 0, 2, 0, fake, None, None) == -1 and "n_seqs" in msg()
    assert topk(fake, None, arr, 129, 2, 0, fake, None, None) == -1 and "n_seqs" in msg()
    assert topk(fake, fake, L.int_array([3, 0]), 2, 2, 1, fake, None, None) == -1 and "sequence 1" in msg()
    assert topk(fake, None, L.int_array([1 << 20, 1]), 2, 1, 0, fake, None, None) == -1 and "2^20" in msg()
    assert "ivosw_brain_topk_ragged" in msg()


# ---------------------------------------------------------------------------------------------- the host half with k > 1
def test_merge_candidates():
    rank = np.array([4, 2, 7, 0, -1, -1])
    assert merge_candidates(None, rank, 6).tolist() == [4, 2, 7, 0] and merge_candidates(None, rank, 3).tolist() == [4, 2, 7]
    assert merge_candidates(7, rank, 4).tolist() == [7, 4, 2, 0]                          # the pick first, removed from the rest
    assert merge_candidates(9, rank[:3], 3).tolist() == [9, 4, 2]                         # a pick outside the ranking: cut to k
    assert merge_candidates(4, rank, 2).tolist() == [4, 2]
    assert merge_candidates(np.int64(0), np.array([0, -1, -1]), 3).tolist() == [0]        # a one-frame sequence
    assert merge_candidates(3, rank, 4).dtype == np.int64


def _stand_in(agent, calls):
    """Replaces the device half: the ranking of a state is the rising order of its first column."""
    def ranked(states, k=None, skip_annotated=None, out=None):
        calls.append(len(states))
        rank = torch.full((len(states), k), -1, dtype=torch.int64)
        for i, s in enumerate(states):
            order = np.argsort(np.asarray(s.cpu() if torch.is_tensor(s) else s)[:, 0], kind="stable")[:k]
            rank[i, :len(order)] = torch.from_numpy(order)
        if out is not None:
            out.view(len(states), k).copy_(rank)
            return out
        return rank
    agent.candidates_device = ranked
    agent.greedy_index_device = agent.greedy_indices_device = None          # the argmax path is not taken


@pytest.mark.parametrize("phase", ["train", "eval"])
@pytest.mark.parametrize("k", [3, 16])
def test_actions_with_candidates_moves_the_host_state_like_sequential_action_calls(phase, k, capsys):
    rs = np.random.RandomState(5)
    states = [np.stack([rs.rand(n), rs.randint(0, 3, n).astype(np.float64)], 1) for n in (7, 12, 5, 9, 30, 2)]
    a, b, plain = (Agent("cpu", _cfg(phase, candidates=k, skip_annotated=True)) for _ in range(3))
    plain.candidates, plain.skip_annotated = 1, False                   # the reference's host half
    plain.greedy_index_device = lambda st, out=None: torch.zeros(1, dtype=torch.int64)
    for ag in (a, b, plain):
        ag.steps_done = 40
    ca, cb = [], []
    _stand_in(a, ca)
    _stand_in(b, cb)
    runs = []
    for run in (lambda: [plain.action(s) for s in states], lambda: [a.action(s) for s in states], lambda: b.actions(states)):
        random.seed(2)
        np.random.seed(2)
        res = run()
        runs.append((res, capsys.readouterr().out, random.random(), float(np.random.rand())))
    (ref, log_ref, *rng_ref), (want, log_want, *rng_want), (got, log_got, *rng_got) = runs
    assert log_ref == log_want == log_got and log_got.count("step:") == 6
    assert rng_ref == rng_want == rng_got
    assert plain.steps_done == a.steps_done == b.steps_done == 46
    assert ca == [1] * 6 and cb == [6]                                  # ONE device call for all states under `actions`
    randomly = ["randomly" in ln for ln in log_ref.splitlines()]
    assert (0 < sum(randomly) < 6) if phase == "train" else not any(randomly)
    for s, r, w, g, rnd in zip(states, ref, want, got, randomly):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and g.tolist() == w.tolist()
        n = len(s)
        assert len(g) == min(k, n) and len(set(g.tolist())) == len(g) and all(0 <= i < n for i in g)
        order = np.argsort(s[:, 0], kind="stable")
        if rnd:                                                         # the reference's random pick first, then the ranking without it
            assert int(g[0]) == int(r) and g[1:].tolist() == [int(i) for i in order if int(i) != int(r)][:min(k, n) - 1]
        else:
            assert g.tolist() == order[:k].tolist()


def test_action_with_skip_annotated_alone_keeps_its_types(capsys):
    a = Agent("cpu", _cfg("train", skip_annotated=True))
    calls = []
    _stand_in(a, calls)
    state = np.stack([np.array([3., 1., 2.]), np.zeros(3)], 1)
    random.seed(1)
    a.EPS_START = a.EPS_END = 0.0                                       # greedy
    got = a.action(state, verbose=False)
    assert isinstance(got, np.int64) and int(got) == 1 and calls == [1]
    assert [int(v) for v in a.actions([state, state[::-1].copy()], verbose=False)] == [1, 1] and calls == [1, 2]
    a.EPS_START = a.EPS_END = 2.0                                       # every draw is random: no device call with one candidate
    got = a.action(state, verbose=False)
    assert 0 <= int(got) < 3 and calls == [1, 2]
    assert all(0 <= int(v) < 3 for v in a.actions([state, state], verbose=False)) and calls == [1, 2]
    out = torch.full((2, 1), -1, dtype=torch.int64)                     # device_out: the ranking stays there, None marks a greedy state
    a.EPS_START = a.EPS_END = 0.0
    assert a.actions([state, state[::-1].copy()], verbose=False, device_out=out) == [None, None] and out.tolist() == [[1], [1]]


def test_worst_candidates_walk_select_next_frame_order():
    q = np.array([0.5, 0.1, 0.9, 0.3, 0.7])
    assert utils_agent.worst_candidates(q, 3, None).tolist() == [1, 3, 0]
    assert utils_agent.worst_candidates(q, 3, [1, 0]).tolist() == [3, 4, 2]
    assert utils_agent.worst_candidates(q, 5, [1, 0]).tolist() == [3, 4, 2, 1, 0]
    assert utils_agent.worst_candidates(q, 2, [0, 1, 2, 3, 4]).tolist() == [1, 3]         # every frame annotated: the fallback's argmin first
    for prev in (None, [1, 0], [0, 1, 2, 3, 4]):
        assert int(utils_agent.worst_candidates(q, 1, prev)[0]) == int(utils_agent.select_next_frame(q, "worst", prev))
    cy = AD(setting="oracle", method="worst", agent=AD(candidates=3))
    req = dict(n_frame=5, n_objects=1, all_F=None, all_P=None, new_masks_quality=q, prev_frames=[1], annotated_frames_list=[1],
               mask_quality=None, first_frame=1, max_nb_interactions=8)
    assert [c.tolist() for c in utils_agent.recommend_candidates(cy, None, None, "cpu", [req, req])] == [[3, 0, 4]] * 2
    assert [int(i) for i in utils_agent.recommend_frames(cy, None, None, "cpu", [req])] == [3]
