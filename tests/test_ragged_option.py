"""The ragged Brain entries, the parts that need no GPU: the host-side row count and refusals of the C ABI, and the host half of
Agent.actions (steps_done, the epsilon threshold, the two host RNG streams) against sequential Agent.action calls."""
import copy
import ctypes
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.models.agent import Agent


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _ints(*v):
    return L.int_array(v)


def test_ragged_rows_is_the_sum_of_the_lengths(lib):
    assert L.MAX_SEQS == 128
    assert lib.ivosw_brain_ragged_rows(_ints(7), 1) == 7
    assert lib.ivosw_brain_ragged_rows(_ints(1, 2, 3, 47, 48, 49, 63, 64, 65), 9) == 342
    assert lib.ivosw_brain_ragged_rows(_ints(*[1 + k % 4 for k in range(128)]), 128) == 320
    assert lib.ivosw_brain_ragged_rows(_ints(1 << 19, 1 << 19), 2) == 1 << 20            # 2^20 rows are still taken
    assert lib.ivosw_brain_ragged_ws_bytes(342) > 342 * (128 + 128 + 512 + 256 + 128) * 4
    assert lib.ivosw_brain_ragged_ws_bytes(0) == 0 and lib.ivosw_brain_ragged_ws_bytes((1 << 20) + 1) == 0


def _fwd_buffers(N, T, nkeep):
    """The forward workspace's buffers in floats: a1, e, gx, hs, d1, q, then gates, cs, hprev of the kept samples."""
    r = N * T
    kept = [2 * nkeep * T * 512, 2 * nkeep * T * 128, 2 * nkeep * T * 128] if nkeep else []
    return [r * 128, r * 128, r * 512, r * 256, r * 128, r] + kept


def _dqn_buffers(B, T):
    """The DQN step's: the policy pass on [s'; s] keeping s, the target pass, xcat, dq, dd1c, w4term, hcc, dhc, dG, dgx, de, da1 and the
    four slab sets (dW2: 16, dW_hh and dW_ih: 40 each, of 512 x 128; the row-split column sums: 8 x 512)."""
    r = B * T
    return (_fwd_buffers(2 * B, T, B) + _fwd_buffers(B, T, 0) + [2 * r * 2, B, B * 128, B * 128, B * 256, B * 256, 2 * r * 512, r * 512,
                                                                  r * 128, r * 128, 16 * 65536, 40 * 65536, 40 * 65536, 8 * 512])


FWD_SLACK, DQN_SLACK = 64 * 16, 64 * 32      # floats the size formulas used to add per forward pass / per step for the 256-byte alignment


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (5, 25), (128, 25)])
def test_workspace_queries_are_the_end_of_the_carve(lib, B, T):
    """Every size query is positive, a multiple of 256, not below the plain sum of its buffers and not above what the earlier formula
    (that sum + slack constants) gave."""
    for got, bufs, slack in ((lib.ivosw_brain_ws_bytes(B, T), _fwd_buffers(B, T, 0), FWD_SLACK),
                             (lib.ivosw_dqn_ws_bytes(B, T), _dqn_buffers(B, T), 2 * FWD_SLACK + DQN_SLACK)):
        assert got > 0 and got % 256 == 0
        assert 4 * sum(bufs) <= got <= 4 * (sum(bufs) + slack), (got, 4 * sum(bufs))


@pytest.mark.parametrize("rows", [1, 342])
def test_ragged_workspace_query_is_the_end_of_the_carve(lib, rows):
    got, bufs = lib.ivosw_brain_ragged_ws_bytes(rows), _fwd_buffers(1, rows, 0)
    assert got > 0 and got % 256 == 0
    assert 4 * sum(bufs) <= got <= 4 * (sum(bufs) + FWD_SLACK)
    assert got == lib.ivosw_brain_ws_bytes(1, rows)             # the flat rows are one [1, R] batch


def test_workspace_queries_refuse_as_before(lib):
    for B, T in ((0, 25), (-1, 25), (5, 0), (5, -3)):
        assert lib.ivosw_brain_ws_bytes(B, T) == 0 and lib.ivosw_dqn_ws_bytes(B, T) == 0
    assert lib.ivosw_brain_ragged_ws_bytes(0) == 0 and lib.ivosw_brain_ragged_ws_bytes(-4) == 0
    assert lib.ivosw_brain_ragged_ws_bytes(1 << 20) > 0 and lib.ivosw_brain_ragged_ws_bytes((1 << 20) + 1) == 0


def test_ragged_rows_refusals_name_the_sequence(lib):
    msg = lambda: lib.ivosw_last_error().decode()
    good = [3, 5, 4]
    assert lib.ivosw_brain_ragged_rows(None, 3) == -1 and "null pointer" in msg()
    for n in (0, 129, -1):
        assert lib.ivosw_brain_ragged_rows(_ints(*([2] * 129)), n) == -1 and "n_seqs" in msg() and str(n) in msg()
    assert lib.ivosw_brain_ragged_rows(_ints(3, 0, 4), 3) == -1 and "sequence 1" in msg() and "positive" in msg()
    assert lib.ivosw_brain_ragged_rows(_ints(3, 5, -2), 3) == -1 and "sequence 2" in msg()
    assert lib.ivosw_brain_ragged_rows(_ints(1 << 19, 1 << 19, 1), 3) == -1 and "sequence 2" in msg() and "2^20" in msg()
    assert lib.ivosw_brain_ragged_rows(_ints(*good), 3) == 12


def test_device_entries_refuse_null_pointers_without_touching_the_gpu(lib):
    msg = lambda: lib.ivosw_last_error().decode()
    arr = _ints(3, 5)
    fake = ctypes.c_void_p(0x10000)                                 # a made-up address: a refused call dereferences nothing
    assert lib.ivosw_brain_forward_ragged(None, None, None, 2, None, None, 0, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_brain_forward_ragged(fake, fake, None, 2, fake, fake, 1 << 30, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_brain_forward_ragged(fake, fake, arr, 2, None, fake, 1 << 30, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_brain_argmax_ragged(None, arr, 2, None, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_brain_argmax_ragged(fake, None, 2, fake, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_quality_state_ragged(None, arr, arr, 2, None, None, None, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_quality_state_ragged(fake, None, arr, 2, fake, fake, fake, None) == -1 and "null pointer" in msg()
    # the lengths are checked before any device is looked up: the same refusals as the host-only query, the entry named
    assert lib.ivosw_brain_forward_ragged(fake, fake, arr, 0, fake, fake, 1 << 30, None) == -1 and "n_seqs" in msg()
    assert lib.ivosw_brain_forward_ragged(fake, fake, _ints(3, 0), 2, fake, fake, 1 << 30, None) == -1 and "sequence 1" in msg()
    assert "ivosw_brain_forward_ragged" in msg()
    assert lib.ivosw_brain_argmax_ragged(fake, arr, 129, fake, None) == -1 and "n_seqs" in msg()
    assert lib.ivosw_brain_argmax_ragged(fake, _ints(0, 2), 2, fake, None) == -1 and "sequence 0" in msg()
    assert lib.ivosw_quality_state_ragged(fake, arr, _ints(3, -1), 2, fake, fake, fake, None) == -1 and "sequence 1" in msg()
    assert lib.ivosw_quality_state_ragged(fake, _ints(2, 0), arr, 2, fake, fake, fake, None) == -1 and "sequence 1" in msg() and "n_obj" in msg()
    assert lib.ivosw_quality_state_ragged(fake, arr, _ints(1 << 20, 1), 2, fake, fake, fake, None) == -1 and "2^20" in msg()


# ---------------------------------------------------------------------------------------------- Agent.actions, the host half
def _agent(phase):
    cfg = AD(phase=phase, data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                          update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    return Agent("cpu", cfg)


def _stand_in(agent, calls):
    """Replaces the device half of an agent: the greedy index of a state is the argmin of its first column."""
    def one(state, out=None):
        calls.append(("one", 1))
        return torch.tensor([int(np.argmin(np.asarray(state)[:, 0]))], dtype=torch.int64)

    def many(states, out=None):
        calls.append(("many", len(states)))
        idx = torch.tensor([int(np.argmin(np.asarray(s)[:, 0])) for s in states], dtype=torch.int64)
        if out is not None:
            out.copy_(idx)
            return out
        return idx
    agent.greedy_index_device, agent.greedy_indices_device = one, many


@pytest.mark.parametrize("phase", ["train", "eval"])
def test_actions_moves_the_host_state_like_sequential_action_calls(phase, capsys):
    rs = np.random.RandomState(5)
    states = [np.stack([rs.rand(n), rs.randint(0, 3, n).astype(np.float64)], 1) for n in (7, 12, 5, 9, 30, 4)]
    a, b = _agent(phase), _agent(phase)
    a.steps_done = b.steps_done = 40
    ca, cb = [], []
    _stand_in(a, ca)
    _stand_in(b, cb)
    random.seed(2)
    np.random.seed(2)
    want = [a.action(s) for s in states]
    log_want = capsys.readouterr().out
    after_want = (random.random(), float(np.random.rand()))
    random.seed(2)
    np.random.seed(2)
    got = b.actions(states)
    log_got = capsys.readouterr().out
    after_got = (random.random(), float(np.random.rand()))
    greedy = [kind == "one" for kind, _ in ca]
    if phase == "train":                                                # the seed mixes both branches
        assert 0 < len(ca) < 6 and log_want.count("randomly") == 6 - len(ca) and log_want.count("by agent") == len(ca)
    else:
        assert len(ca) == 6 and "randomly" not in log_want
    assert cb == [("many", 6)]                                          # ONE device call for all states
    assert [int(v) for v in got] == [int(v) for v in want] and all(0 <= int(v) < len(s) for v, s in zip(got, states))
    assert log_got == log_want and log_got.count("step:") == 6
    assert a.steps_done == b.steps_done == 46
    assert after_got == after_want
    # with device_out the greedy entries stay on the device (None), the random picks are host integers
    c = _agent(phase)
    c.steps_done = 40
    cc = []
    _stand_in(c, cc)
    random.seed(2)
    np.random.seed(2)
    out = torch.full((6,), -1, dtype=torch.int64)
    kept = c.actions(states, verbose=False, device_out=out)
    assert capsys.readouterr().out == ""
    mask = ["by agent" in ln for ln in log_want.splitlines()]
    assert len(mask) == 6 and sum(mask) == len(greedy)
    for k, (pk, w, g) in enumerate(zip(kept, want, mask)):
        if g:
            assert pk is None and int(out[k]) == int(w)
        else:
            assert pk is not None and int(pk) == int(w)
    assert c.steps_done == 46 and (random.random(), float(np.random.rand())) == after_want


def test_actions_without_a_greedy_state_makes_no_device_call():
    a = _agent("train")
    a.EPS_START = a.EPS_END = 2.0                                       # every draw is below the threshold: all random
    calls = []
    _stand_in(a, calls)
    random.seed(0)
    got = a.actions([np.zeros((4, 2)), np.zeros((9, 2))], verbose=False)
    assert calls == [] and all(p is not None for p in got) and 0 <= int(got[0]) < 4 and 0 <= int(got[1]) < 9
    assert a.actions([], verbose=False) == [] and a.steps_done == 2
