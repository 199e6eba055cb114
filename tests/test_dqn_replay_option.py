"""The prioritized-replay option (cfg.agent.replay = "uniform" | "prioritized", per_alpha, per_beta, per_beta_steps, per_eps) on the host side,
no GPU: the CLI and YAML carry it, the agent refuses what it cannot run, the C ABI refuses bad arguments before it touches a pointer, the
host mirror of the sum-tree draw is an fp64 cumulative-sum search, and the host mirror of the priority update keeps the duplicate-slot rule
and the full-rebuild identity."""
import ctypes

import numpy as np
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models import momory_pool as mp


class AD(dict):
    __getattr__ = dict.__getitem__


def test_defaults_and_cli_carry_the_replay_option(tmp_path):
    c = entry.parse_cli([])
    assert (c.agent.replay, c.agent.per_alpha, c.agent.per_beta, c.agent.per_beta_steps, c.agent.per_eps) == ("uniform", 0.6, 0.4, 0, 1e-6)
    c = entry.parse_cli(["with", "agent.replay=prioritized", "agent.per_alpha=0.7", "agent.per_beta_steps=500"])
    assert (c.agent.replay, c.agent.per_alpha, c.agent.per_beta_steps) == ("prioritized", 0.7, 500)
    assert isinstance(c.agent.per_beta_steps, int)
    p = tmp_path / "cfg.yaml"
    p.write_text("agent:\n  replay: prioritized\n  per_beta: 0.5\n")
    c = entry.parse_cli(["--config", str(p)])
    assert (c.agent.replay, c.agent.per_beta, c.agent.per_alpha, c.agent.gamma) == ("prioritized", 0.5, 0.6, 0.95)


def test_agent_reads_the_option_and_refuses_the_unknown():
    from ivos_w_amd.models.agent import Agent, replay_option
    opt = Agent._replay_option
    assert opt(AD(gamma=0.95)) == ("uniform", None, None, None, None)          # configs without the keys keep uniform minibatches
    assert opt(AD(entry.parse_cli([]).agent)) == ("uniform", None, None, None, None)
    assert opt(AD(replay="uniform", per_alpha="junk", per_eps=-1)) == ("uniform", None, None, None, None)   # only checked under PER
    assert opt(AD(replay="prioritized")) == ("prioritized", 0.6, 0.4, 0, 1e-6)
    assert opt(AD(replay="prioritized", per_alpha=0, per_beta=1, per_beta_steps=7, per_eps=2)) == ("prioritized", 0.0, 1.0, 7, 2.0)
    assert replay_option("prioritized", 1, 0, 0, 1e-3) == ("prioritized", 1.0, 0.0, 0, 1e-3)
    P = dict(replay="prioritized")
    for bad in (dict(replay="Prioritized"), dict(replay="per"), dict(replay=None), dict(replay=1), dict(replay="UNIFORM"),
                dict(P, per_alpha=-0.1), dict(P, per_alpha=float("nan")), dict(P, per_alpha=float("inf")), dict(P, per_alpha="0.6"),
                dict(P, per_alpha=True), dict(P, per_alpha=None),
                dict(P, per_beta=-0.01), dict(P, per_beta=1.01), dict(P, per_beta=float("nan")), dict(P, per_beta="0.4"), dict(P, per_beta=False),
                dict(P, per_beta_steps=-1), dict(P, per_beta_steps=10.0), dict(P, per_beta_steps="10"), dict(P, per_beta_steps=True),
                dict(P, per_beta_steps=2 ** 31),
                dict(P, per_eps=0), dict(P, per_eps=-1e-6), dict(P, per_eps=float("inf")), dict(P, per_eps=float("nan")), dict(P, per_eps=1e-50),
                dict(P, per_eps="1e-6")):
        with pytest.raises(ValueError):
            opt(AD(bad))


def test_the_entries_are_bound():
    S = L.SIGNATURES
    for name in ("ivosw_per_build", "ivosw_per_draw_gather", "ivosw_per_update", "ivosw_dqn_loss_grad_per"):
        assert S[name][0] is L._i, name
    assert S["ivosw_per_state_bytes"] == (L._sz, []) and S["ivosw_per_tree_floats"] == (L._sz, [L._i])
    ex = S["ivosw_dqn_loss_grad_ex"][1]
    assert S["ivosw_dqn_loss_grad_per"][1] == ex[:12] + [L._p, L._p] + ex[12:]        # weights, td_out after huber_delta


def test_host_queries_of_the_library():
    lib = L.lib()
    assert lib.ivosw_per_state_bytes() == 32
    assert lib.ivosw_version() == 102
    for n, P in ((1, 2), (2, 2), (3, 4), (50000, 65536), (65536, 65536), (1 << 24, 1 << 24)):
        assert lib.ivosw_per_tree_floats(n) == 2 * P == 2 * mp.per_tree_leaves(n), n
    assert lib.ivosw_per_tree_floats(0) == 0 and lib.ivosw_per_tree_floats((1 << 24) + 1) == 0 and lib.ivosw_per_tree_floats(-3) == 0


def test_argument_errors_do_not_touch_the_gpu():
    """Every refusal returns IVOSW_ERR_ARG before a pointer is dereferenced or a launch made: the pointers here are bogus host addresses."""
    lib = L.lib()
    x = ctypes.c_void_p(16)
    ERR = -1

    def build(tree=x, n=100, old=None, n_old=0, st=x, alpha=0.6):
        return lib.ivosw_per_build(tree, n, old, n_old, st, alpha, None)

    for kw in (dict(tree=None), dict(st=None), dict(n=0), dict(n=-1), dict(n=(1 << 24) + 1), dict(n_old=-1), dict(n_old=101, old=x),
               dict(n_old=5), dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        assert build(**kw) == ERR, kw

    def draw(cols=x, tree=x, st=x, n=100, B=32, T=25, beta0=0.4, steps=0, outs=x, weights=x):
        return lib.ivosw_per_draw_gather(cols, x, x, x, x, x, x, tree, st, n, B, T, beta0, steps, outs, weights, x, x, x, x, x, None)

    for kw in (dict(cols=None), dict(tree=None), dict(st=None), dict(outs=None), dict(weights=None), dict(n=0), dict(n=(1 << 24) + 1),
               dict(B=0), dict(B=1025), dict(T=0), dict(beta0=-0.1), dict(beta0=1.5), dict(beta0=float("nan")), dict(steps=-1)):
        assert draw(**kw) == ERR, kw

    def update(tree=x, n=100, st=x, idx=x, td=x, B=32, alpha=0.6, eps=1e-6):
        return lib.ivosw_per_update(tree, n, st, idx, td, B, alpha, eps, None)

    for kw in (dict(tree=None), dict(st=None), dict(idx=None), dict(td=None), dict(n=0), dict(n=(1 << 24) + 1), dict(B=0), dict(B=2000),
               dict(alpha=-1.0), dict(alpha=float("nan")), dict(eps=0.0), dict(eps=-1e-6), dict(eps=float("inf")), dict(eps=float("nan"))):
        assert update(**kw) == ERR, kw

    def loss(weights=x, td=x, grads=x):
        return lib.ivosw_dqn_loss_grad_per(x, x, x, x, x, x, x, 32, 25, 0.95, 0, 1.0, weights, td, grads, x, x, 10, None)

    for kw in (dict(weights=None), dict(td=None), dict(grads=None)):
        assert loss(**kw) == ERR, kw
    assert b"null" in lib.ivosw_last_error()


def _random_tree(rng, n, spread=3.0):
    P = mp.per_tree_leaves(n)
    t = np.zeros(2 * P, dtype=np.float32)
    t[P:P + n] = np.exp(rng.uniform(-spread, spread, n)).astype(np.float32)
    return mp.per_rebuild(t)


@pytest.mark.parametrize("n,B", [(1000, 64), (50000, 128), (3, 7), (1, 4), (4096, 1)])
def test_per_draw_rows_is_the_cumulative_sum_search(n, B):
    """Slot b lands on the row whose fp64 cumulative-sum interval holds x_b = total * (b + u_b) / B; targets near an
    interval boundary (1e-6 of the total) are skipped (fp32 partial sums move them)."""
    rng = np.random.default_rng(n + B)
    for trial in range(4):
        t = _random_tree(rng, n)
        P = t.shape[0] // 2
        leaves = t[P:P + n].astype(np.float64)
        cum = np.cumsum(leaves)
        total = cum[-1]
        seed, counter = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32))
        rows = mp.per_draw_rows(t, seed, counter, B, n)
        assert rows.shape == (B,) and rows.min() >= 0 and rows.max() < n
        checked = 0
        for b in range(B):
            u = (mp._draw_mix(seed, counter, b) >> 40) * 2.0 ** -24
            x = total * (b + u) / B
            want = int(np.searchsorted(cum, x, side="right"))
            if np.abs(cum - x).min() < 1e-6 * total or want >= n:
                continue
            assert rows[b] == want, (trial, b)
            checked += 1
        assert checked >= 0.8 * B or B < 8


def test_per_draw_rows_is_stratified_and_uniform_when_flat():
    """Equal leaves: slot b falls in the b-th of B equal strata of the rows."""
    n, B = 1024, 128
    P = mp.per_tree_leaves(n)
    t = np.zeros(2 * P, dtype=np.float32)
    t[P:P + n] = 1.0
    t = mp.per_rebuild(t)
    rows = mp.per_draw_rows(t, 99, 3, B, n)
    assert np.array_equal(rows // (n // B), np.arange(B))


def test_per_beta_anneals_linearly():
    assert mp.per_beta(0.4, 0, 10 ** 6) == np.float32(0.4)
    assert mp.per_beta(0.4, 100, 0) == np.float32(0.4)
    assert mp.per_beta(0.4, 100, 100) == np.float32(1.0) == mp.per_beta(0.4, 100, 2 ** 32 - 1)
    vals = [float(mp.per_beta(0.4, 100, c)) for c in range(101)]
    assert all(a < b for a, b in zip(vals, vals[1:]))
    np.testing.assert_allclose(vals, 0.4 + 0.6 * np.arange(101) / 100, rtol=1e-6)


def test_host_update_duplicate_rule_and_full_rebuild_identity():
    rng = np.random.default_rng(5)
    n = 777
    t0 = _random_tree(rng, n)
    P = t0.shape[0] // 2
    idx = np.array([5, 9, 5, 700, 9, 776, 5, 0, -1, n], dtype=np.int64)        # repeated rows, and two outside [0, n)
    td = rng.uniform(0, 2, idx.size).astype(np.float32)
    t1, mx = mp.per_update_host(t0, 1.0, idx, td, 0.6, 1e-6, n)
    p = td + np.float32(1e-6)
    for r, b in ((5, 6), (9, 4), (700, 3), (776, 5), (0, 7)):                 # the highest slot of a row wins
        assert t1[P + r] == np.power(p[b], np.float32(0.6), dtype=np.float32), r
    untouched = np.setdiff1d(np.arange(n), [0, 5, 9, 700, 776])
    np.testing.assert_array_equal(t1[P + untouched], t0[P + untouched])
    np.testing.assert_array_equal(t1, mp.per_rebuild(t1))                     # every internal node == left + right
    assert t1[0] == 0 and mx == np.float32(max(1.0, p.max()))
    _, mx2 = mp.per_update_host(t0, 5.0, idx, td, 0.6, 1e-6, n)
    assert mx2 == np.float32(5.0)


def test_prioritized_loop_refuses_what_it_cannot_run(monkeypatch):
    """Under an initialised process group, IVOSW_UPDATE_PATH=host or a foreign loader the prioritized episode loop refuses with the reason
    (before any GPU work)."""
    from torch.utils.data import DataLoader

    from ivos_w_amd.datasets.agent_dataset import DAVIS2017AgentTrain
    from ivos_w_amd.models.agent import Agent
    from ivos_w_amd.utils import utils_agent
    agent = object.__new__(Agent)
    agent.__dict__.update(replay_kind="prioritized", device="cuda:0", per_replay=None)
    ds = DAVIS2017AgentTrain.from_soa(dict(action=np.zeros(4, np.int64), old_state_iou=np.zeros((4, 3)), new_state_iou=np.zeros((4, 3)),
                                           annotated_frames=np.zeros((4, 3)), next_annotated_frames=np.zeros((4, 3)),
                                           reward_step=np.zeros(4), reward_done=np.zeros(4), done=np.zeros(4, bool)))
    loader = DataLoader(ds, batch_size=2, shuffle=True, num_workers=0)
    monkeypatch.setattr(Agent, "_world", staticmethod(lambda: (object(), 2)))
    with pytest.raises(ValueError, match="torch.distributed"):
        utils_agent._device_update_loop(agent, loader, 10)
    monkeypatch.setattr(Agent, "_world", staticmethod(lambda: (None, 1)))
    monkeypatch.setenv("IVOSW_UPDATE_PATH", "host")
    with pytest.raises(ValueError, match="IVOSW_UPDATE_PATH"):
        utils_agent._device_update_loop(agent, loader, 10)
    monkeypatch.delenv("IVOSW_UPDATE_PATH")
    with pytest.raises(ValueError, match="plain DataLoader"):
        utils_agent._device_update_loop(agent, [dict(action=np.zeros(2))], 10)
    with pytest.raises(ValueError, match="plain DataLoader"):
        utils_agent._device_update_loop(agent, DataLoader(ds, batch_size=2, collate_fn=lambda b: b), 10)
