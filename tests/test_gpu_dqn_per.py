"""GPU: prioritized experience replay (cfg.agent.replay = "prioritized") through every layer that carries it - the sum-tree build, the draw +
gather, the importance-weighted head kernels (fused chain and DQN_FUSED=0), the priority update, PrioritizedReplay, Agent.loss_and_grads,
CapturedDqnStep / GraphedDqnLoop with the composed chain, and train_agent.py.  Yardsticks: the host mirrors of momory_pool (per_draw_rows,
per_rebuild, per_beta), fp64 restatements of the weights and of the weighted loss (oracle/brain_oracle.py), and the unweighted entries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ivos_w_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AD(dict):
    __getattr__ = dict.__getitem__


def cfg(update_rate=0.5, **agent):
    base = dict(memory_size=1000, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500, update_rate=update_rate, lr=5e-6,
                weight_decay=5e-4, replay="prioritized")
    base.update(agent)
    return AD(phase="train", data=AD(subset="train"), agent=AD(base))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def load_brain(net, seed):
    sd = synth.brain_state_dict(seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def make_agent(dev, **agent):
    from ivos_w_amd.models.agent import Agent
    a = Agent(dev, cfg(**agent))
    load_brain(a.policy_net, 0)
    load_brain(a.target_net, 1)
    return a


def replay_with_leaves(dev, tr, leaves, seed=7, **per):
    """A PrioritizedReplay over `tr` whose leaves are `leaves` (carried over by ivosw_per_build from a device array)."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    rp = PrioritizedReplay(tr, dev, seed=seed, **per)
    old = torch.from_numpy(np.asarray(leaves, dtype=np.float32)).to(dev)
    L.check(L.lib().ivosw_per_build(L.dptr(rp.tree), rp.n, L.dptr(old), rp.n, L.dptr(rp.state), float(np.float32(rp.alpha)),
                                    L.stream_ptr(dev)), "per_build")
    return rp


def ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------------------------------------------------- build
def test_build_fresh_and_with_carry_over(dev):
    from ivos_w_amd.models.momory_pool import PrioritizedReplay, per_rebuild
    tr = synth.replay_transitions(n=5000, T=25, seed=3)
    rp = PrioritizedReplay(tr, dev, alpha=0.6, seed=1)
    t = rp.tree_host()
    P = rp.P
    assert P == 8192 and t.shape == (2 * P,)
    assert np.all(t[P:P + 5000] == 1.0) and np.all(t[P + 5000:] == 0) and t[0] == 0
    np.testing.assert_array_equal(t.view(np.uint32), per_rebuild(t).view(np.uint32))
    assert t[1] == 5000.0 and rp.counter() == 0 and rp.max_priority() == 1.0
    # random leaves, then a max_priority of 2.5 and a reload with 3000 more rows: the old leaves stay, the new rows get 2.5 ** alpha
    rng = np.random.default_rng(0)
    leaves = rng.uniform(0.01, 3.0, 5000).astype(np.float32)
    rp = replay_with_leaves(dev, tr, leaves, alpha=0.6)
    rp.state[16:20].copy_(torch.from_numpy(np.array([2.5], np.float32).view(np.uint8)))
    rp.set_counter(41)
    t = rp.tree_host()
    np.testing.assert_array_equal(t.view(np.uint32), per_rebuild(t).view(np.uint32))
    extra = synth.replay_transitions(n=3000, T=25, seed=9)
    more = {k: np.concatenate([tr[k], extra[k]]) for k in tr}
    rb = rp.rebuilt(more)
    t2 = rb.tree_host()
    assert rb.carried == 5000 and rb.counter() == 41 and rb.max_priority() == 2.5 and rb.seed == rp.seed
    np.testing.assert_array_equal(t2[rb.P:rb.P + 5000], leaves)
    new = t2[rb.P + 5000:rb.P + 8000]
    assert np.all(new == new[0]) and ulps(new[0], 2.5 ** np.float64(np.float32(0.6))) <= 2
    np.testing.assert_array_equal(t2.view(np.uint32), per_rebuild(t2).view(np.uint32))
    # not a prefix: every leaf starts again from max_priority ** alpha
    other = synth.replay_transitions(n=6000, T=25, seed=4)
    ro = rp.rebuilt(other)
    lv = ro.leaves()
    assert ro.carried == 0 and np.all(lv == lv[0]) and ulps(lv[0], 2.5 ** np.float64(np.float32(0.6))) <= 2
    for a in (0.0, 1.0):
        r0 = PrioritizedReplay(tr, dev, alpha=a)
        assert np.all(r0.leaves() == 1.0)


# -------------------------------------------------------------------------------------------------------------------------------- draw
def test_draw_matches_the_host_mirror_gather_and_weights(dev):
    from ivos_w_amd.models.momory_pool import DeviceReplay, per_beta, per_draw_rows
    n, B = 50000, 128
    tr = synth.replay_transitions(n=n, T=25, seed=5)
    rng = np.random.default_rng(1)
    leaves = np.exp(rng.uniform(-4, 4, n)).astype(np.float32)
    rp = replay_with_leaves(dev, tr, leaves, seed=0x1234_5678_9ABC, alpha=0.6, beta0=0.4, beta_steps=40)
    plain = DeviceReplay(tr, dev)
    t = rp.tree_host()
    total = np.float64(t[1])
    out = rp.new_batch(B)
    for c in range(64):
        assert rp.counter() == c
        beta = float(per_beta(0.4, 40, c))
        assert rp.beta_next() == beta
        rp.sample_prioritized(B, out=out)
        idx = out["idx"].cpu().numpy()
        np.testing.assert_array_equal(idx, per_draw_rows(t, rp.seed, c, B, n))
        ref = plain.sample(out["idx"])
        for k in ("state", "new_state", "action", "reward_step", "reward_done"):
            assert torch.equal(out[k], ref[k]), (c, k)
        w = out["weights"].cpu().numpy().astype(np.float64)
        w64 = (leaves[idx].astype(np.float64) * n / total) ** -beta
        w64 /= w64.max()
        np.testing.assert_allclose(w, w64, rtol=1e-6)
        assert w.max() == 1.0 and np.all(w > 0)
    assert per_beta(0.4, 40, 40) == 1.0 == per_beta(0.4, 40, 63)
    assert rp.counter() == 64
    np.testing.assert_array_equal(rp.tree_host(), t)                      # the draw reads the tree only


def test_draw_frequencies_follow_the_priorities(dev):
    """One row at 1000x priority among 2000: over 102 400 draws the frequencies of the hot row and of 20 bins of the rest pass a chi-square
    bound (stratified draws vary less than multinomial ones, so the multinomial bound is conservative)."""
    n, B, draws, hot = 2000, 128, 800, 1234
    tr = synth.replay_transitions(n=n, T=4, seed=6)
    leaves = np.ones(n, np.float32)
    leaves[hot] = 1000.0
    rp = replay_with_leaves(dev, tr, leaves, seed=2024, alpha=0.6)
    out = rp.new_batch(B)
    idx = []
    for _ in range(draws):
        rp.sample_prioritized(B, out=out)
        idx.append(out["idx"].clone())
    idx = torch.cat(idx).cpu().numpy()
    p = leaves.astype(np.float64) / leaves.sum()
    cnt = np.bincount(idx, minlength=n)
    rest = np.setdiff1d(np.arange(n), [hot])
    bins = np.array_split(rest, 20)
    obs = np.array([cnt[hot]] + [cnt[b].sum() for b in bins], np.float64)
    exp = np.array([p[hot]] + [p[b].sum() for b in bins]) * idx.size
    chi2 = ((obs - exp) ** 2 / exp).sum()
    assert chi2 < 52.6, (chi2, obs[:4], exp[:4])                      # chi-square, 20 degrees of freedom, p = 1e-4
    assert abs(cnt[hot] / idx.size - p[hot]) < 0.01


# ------------------------------------------------------------------------------------------------------------------------ weighted loss
def _loss_per_vs_ex(agent, sample, weights):
    from ivos_w_amd import _lib as L
    lib = L.lib()
    pn, tn = agent.policy_net, agent.target_net
    B, T, _ = sample["state"].shape
    dev = sample["state"].device
    nbytes = lib.ivosw_dqn_ws_bytes(B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = {}
    for name in ("ex", "per"):
        loss = torch.zeros(1, device=dev)
        td = torch.full((B,), -1.0, device=dev)
        args = [L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(sample["state"]), L.dptr(sample["new_state"]), L.dptr(sample["action"]),
                L.dptr(sample["reward_step"]), L.dptr(sample["reward_done"]), B, T, float(np.float32(agent.GAMMA)), *agent._loss_args()]
        if name == "per":
            args += [L.dptr(weights), L.dptr(td)]
        L.check(getattr(lib, f"ivosw_dqn_loss_grad_{name}")(*args, L.dptr(pn.flat_grad), L.dptr(loss), L.dptr(ws), nbytes,
                                                           L.stream_ptr(dev)), name)
        res[name] = (loss.clone(), pn.flat_grad.clone(), td.clone())
    return res


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("fused", [1, 0])
def test_unit_weights_are_the_unweighted_step_bit_for_bit(dev, loss, fused):
    """alpha = 0: every leaf and every weight is 1, and the weighted head gives the _ex entry's loss and gradients bit for bit."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    tr = synth.replay_transitions(n=3000, T=25, seed=11)
    rp = PrioritizedReplay(tr, dev, alpha=0.0, seed=5)
    agent = make_agent(dev, loss=loss, huber_delta=0.1, per_alpha=0.0)
    try:
        L.tune_set(b"DQN_FUSED", fused)
        for c in range(3):
            s = rp.sample_prioritized(128)
            assert torch.all(s["weights"] == 1.0)
            res = _loss_per_vs_ex(agent, s, s["weights"])
            assert torch.equal(res["ex"][0], res["per"][0]) and torch.equal(res["ex"][1], res["per"][1]), c
            assert torch.all(res["per"][2] >= 0)
            rp.update_priorities(s["idx"], res["per"][2])
            assert np.all(rp.leaves() == 1.0)
    finally:
        L.tune_set(b"DQN_FUSED", 1)


def weighted_step_fp64(P, Pt, batch, w, gamma, kind, delta):
    from oracle import brain_oracle as bo
    state, new_state = bo.build_states(batch, np.float64)
    action = np.asarray(batch["action"]).reshape(-1).astype(np.int64)
    B = action.shape[0]
    y1, y2, _ = bo.dqn_targets(P, Pt, new_state, np.asarray(batch["reward_step"]).reshape(-1), np.asarray(batch["reward_done"]).reshape(-1),
                               gamma, np.float64)
    q, cache = bo.brain_forward(P, state, np.float64, keep=True)
    qsa = q[np.arange(B), action]
    e1, e2 = qsa - y1, qsa - y2
    if kind == "huber":
        h = lambda e: np.where(np.abs(e) < delta, 0.5 * e * e, delta * (np.abs(e) - 0.5 * delta))
        terms, d = h(e1) + h(e2), (np.clip(e1, -delta, delta) + np.clip(e2, -delta, delta)) / B
    else:
        terms, d = e1 * e1 + e2 * e2, 2.0 * (e1 + e2) / B
    dq = np.zeros_like(q)
    dq[np.arange(B), action] = w * d
    return (w * terms).sum() / B, bo.brain_backward(P, cache, dq, np.float64), np.abs(e1) + np.abs(e2)


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("fused", [1, 0])
def test_random_weights_against_fp64(dev, loss, fused):
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.momory_pool import DeviceReplay
    n, B = 500, 128
    tr = synth.replay_transitions(n=n, T=25, seed=11)
    idx = synth.minibatch_indices(0, n=n, B=B, seed=7)
    batch = synth.collate_np(tr, idx)
    w = np.random.default_rng(3).uniform(0.05, 1.0, B).astype(np.float32)
    agent = make_agent(dev, loss=loss, huber_delta=0.1)
    sample = dict(DeviceReplay(tr, dev).sample(torch.from_numpy(idx).to(dev)), weights=torch.from_numpy(w).to(dev),
                  td=torch.empty(B, device=dev))
    try:
        L.tune_set(b"DQN_FUSED", fused)
        got_loss = float(agent.loss_and_grads(sample).item())
    finally:
        L.tune_set(b"DQN_FUSED", 1)
    got = agent.policy_net.flat_grad.cpu().numpy().astype(np.float64)
    loss64, G64, td64 = weighted_step_fp64(synth.brain_state_dict(0), synth.brain_state_dict(1), batch, w.astype(np.float64), 0.95, loss, 0.1)
    np.testing.assert_allclose(got_loss, loss64, rtol=1e-5)
    want = synth.brain_flat(G64).astype(np.float64)
    for k, (off, shp) in synth.brain_offsets().items():
        m = int(np.prod(shp))
        err = np.abs(got[off:off + m] - want[off:off + m]).max() / (np.abs(want[off:off + m]).max() + 1e-30)
        assert err <= 1e-5, (k, err)
    assert agent.last_td is sample["td"]
    np.testing.assert_allclose(sample["td"].cpu().numpy(), td64, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------------ update
def test_priority_update_rules(dev):
    """A 50-row replay drawn 128 at a time: many rows repeat within a draw.  Drawn leaves = powf(td + eps, alpha) of the LAST slot of their
    row, untouched leaves unchanged, every internal node == left + right bit for bit, max_priority = max(old, max(td + eps))."""
    from ivos_w_amd.models.momory_pool import PrioritizedReplay, per_rebuild
    n, B, alpha, eps = 50, 128, 0.7, 1e-3
    tr = synth.replay_transitions(n=n, T=25, seed=8)
    rp = PrioritizedReplay(tr, dev, alpha=alpha, eps=eps, seed=11)
    rng = np.random.default_rng(9)
    for step in range(6):
        before, mx0 = rp.tree_host(), rp.max_priority()
        s = rp.sample_prioritized(B)
        idx = s["idx"].cpu().numpy()
        td = rng.uniform(0, 3, B).astype(np.float32)
        rp.update_priorities(s["idx"], torch.from_numpy(td).to(dev))
        t = rp.tree_host()
        P = rp.P
        last = {int(r): b for b, r in enumerate(idx)}
        assert len(last) < B                                           # duplicates were exercised
        p = td + np.float32(eps)
        for r, b in last.items():
            assert ulps(t[P + r], np.float64(p[b]) ** np.float64(np.float32(alpha))) <= 2, (step, r)
        untouched = np.setdiff1d(np.arange(P), list(last))
        np.testing.assert_array_equal(t[P + untouched], before[P + untouched])
        np.testing.assert_array_equal(t.view(np.uint32), per_rebuild(t).view(np.uint32))
        assert rp.max_priority() == max(mx0, float(p.max()))
    assert rp.max_priority() > 1.0


def test_priority_update_on_a_large_tree(dev):
    """2^17 + 5 rows (18 levels, the last 7 below the draw's LDS levels), random leaves: the update keeps the full-rebuild identity."""
    from ivos_w_amd.models.momory_pool import per_rebuild
    n, B = (1 << 17) + 5, 1024
    tr = synth.replay_transitions(n=n, T=2, seed=1)
    leaves = np.random.default_rng(2).uniform(0.1, 2, n).astype(np.float32)
    rp = replay_with_leaves(dev, tr, leaves, seed=3, alpha=0.5)
    for _ in range(3):
        s = rp.sample_prioritized(B)
        rp.update_priorities(s["idx"], torch.rand(B, device=dev))
        t = rp.tree_host()
        np.testing.assert_array_equal(t.view(np.uint32), per_rebuild(t).view(np.uint32))
    lv = rp.leaves()
    assert (lv != leaves).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------------------- captured
def _eager_chain(agent, rp, B, out):
    rp.sample_prioritized(B, out=out)
    agent.loss_and_grads(out)
    agent.optimizer.step()
    rp.update_priorities(out["idx"], out["td"])


OPTS = {"adam": dict(), "sgd": dict(optimizer="sgd", momentum=0.9, lr=1e-4),
        "adam_poly": dict(lr_schedule="poly", lr_total_steps=10, lr=1e-4)}


@pytest.mark.parametrize("opt", sorted(OPTS))
@pytest.mark.parametrize("steps", [1, 8])
def test_captured_step_equals_the_eager_chain(dev, opt, steps):
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    tr = synth.replay_transitions(n=50000, T=25, seed=2019)
    B, seed = 128, 0xFEED
    kw = dict(OPTS[opt], per_beta_steps=12, loss="huber", huber_delta=0.1)
    ea, ca = make_agent(dev, **kw), make_agent(dev, **kw)
    er = PrioritizedReplay(tr, dev, ea.per_alpha, ea.per_beta, ea.per_beta_steps, ea.per_eps, seed=seed)
    cr = PrioritizedReplay(tr, dev, ca.per_alpha, ca.per_beta, ca.per_beta_steps, ca.per_eps, seed=seed)
    step = CapturedDqnStep(ca, cr, B, fused=True, draw_seed=seed, steps=steps)
    assert step.kernel_nodes > 0
    out = er.new_batch(B)
    for k in range(16 // steps):
        for _ in range(steps):
            _eager_chain(ea, er, B, out)
        step.launch()
        assert torch.equal(ea.policy_net.flat, ca.policy_net.flat), k
        assert torch.equal(er.tree, cr.tree) and torch.equal(er.state, cr.state), k
        assert torch.equal(out["idx"], step.idx) and torch.equal(out["td"], step.td) and torch.equal(ea._loss_dev, step.loss), k
    assert ea.optimizer.state["step"] == ca.optimizer.state["step"] == 16
    for key in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
        if key in ea.optimizer.state:
            assert torch.equal(ea.optimizer.state[key], ca.optimizer.state[key]), key
    assert cr.counter() == 16 and cr.max_priority() == er.max_priority() >= 1.0
    assert (cr.leaves() != 1.0).sum() > 100                            # the drawn rows' priorities moved
    # a changed PER value is refused by the captured step
    cr.alpha = 0.5
    with pytest.raises(RuntimeError, match="per_alpha"):
        step.launch()


def test_graphed_loop_equals_the_step_by_step_loop(dev):
    from ivos_w_amd.models.agent import GraphedDqnLoop, LeanDqnLoop
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    tr = synth.replay_transitions(n=3000, T=25, seed=5)
    B, seed, N = 64, 77, 40
    res = {}
    for mode in ("eager", "graphed", "lean"):
        a = make_agent(dev, update_rate=0.1)
        rp = PrioritizedReplay(tr, dev, a.per_alpha, a.per_beta, a.per_beta_steps, a.per_eps, seed=seed)
        np.random.seed(3)
        if mode == "eager":
            out = rp.new_batch(B)
            for _ in range(N):
                _eager_chain(a, rp, B, out)
                if np.random.random() < a.update_rate:
                    a.sync_target()
        elif mode == "graphed":
            loop = GraphedDqnLoop(a, rp, B, draw_seed=seed, block=8)
            loop.run(N)
        else:
            LeanDqnLoop(a, rp, B, draw_seed=seed).run(N)
        res[mode] = (a.policy_net.flat.clone(), a.target_net.flat.clone(), rp.tree.clone(), rp.state.clone())
    for mode in ("graphed", "lean"):
        for x, y in zip(res["eager"], res[mode]):
            assert torch.equal(x, y), mode


def test_device_update_loop_under_per(dev, capsys):
    """utils_agent._device_update_loop with agent.replay = prioritized: one step per loader batch (capped), the dataset's replay seeded
    from torch's global generator, the same steps as the eager composed chain; a reloaded dataset rebuilds the tree with carry-over."""
    from torch.utils.data import DataLoader
    from ivos_w_amd.datasets.agent_dataset import DAVIS2017AgentTrain
    from ivos_w_amd.utils import utils_agent
    tr = synth.replay_transitions(n=300, T=25, seed=3)
    ds = DAVIS2017AgentTrain.from_soa(tr)
    loader = DataLoader(ds, batch_size=32, shuffle=True, num_workers=0)
    a = make_agent(dev, update_rate=0.2)
    torch.manual_seed(5)
    np.random.seed(5)
    losses = utils_agent._device_update_loop(a, loader, 7)
    assert len(losses) == 7 and a.optimizer.state["step"] == 7
    rp = a.per_replay
    assert rp is ds._per_replay and rp.counter() == 7 and rp.max_priority() >= 1.0 and (rp.leaves() != 1.0).sum() > 32
    # the same steps by hand
    b = make_agent(dev, update_rate=0.2)
    torch.manual_seed(5)
    np.random.seed(5)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    assert seed == rp.seed
    ref = b.prioritized_replay(tr, dev, seed)
    out = ref.new_batch(32)
    for _ in range(7):
        _eager_chain(b, ref, 32, out)
        if np.random.random() < b.update_rate:
            b.sync_target()
    assert torch.equal(a.policy_net.flat, b.policy_net.flat) and torch.equal(a.target_net.flat, b.target_net.flat)
    assert torch.equal(rp.tree, ref.tree) and torch.equal(rp.state, ref.state)
    # a reloaded dataset with more rows: the tree carries over
    extra = synth.replay_transitions(n=100, T=25, seed=9)
    more = {k: np.concatenate([tr[k], extra[k]]) for k in tr}
    ds2 = DAVIS2017AgentTrain.from_soa(more)
    utils_agent._device_update_loop(a, DataLoader(ds2, batch_size=32, shuffle=True, num_workers=0), 2)
    assert a.per_replay is ds2._per_replay and a.per_replay.carried == 300 and a.per_replay.counter() == 9


# --------------------------------------------------------------------------------------------------------------------- train_agent.py
def test_train_agent_with_prioritized_replay(tmp_path):
    script = os.path.join(ROOT, "train_agent.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    res, hists = {}, {}
    for name, opt in (("per", ["agent.replay=prioritized", "agent.per_beta_steps=50"]), ("per2", ["agent.replay=prioritized",
                                                                                                    "agent.per_beta_steps=50"]), ("uniform", [])):
        d = tmp_path / name
        common = ["synthetic=1", "synth.n_sequences=2", "synth.n_frames=26", "synth.height=120", "synth.width=216", f"ckpt_dir={d}/weights",
                  f"report_save_dir={d}/results", f"agent.save_result_dir={d}/train", "num_epochs=1", "agent.train_batch_size=16",
                  "agent.lr=1e-4"]
        r = subprocess.run([sys.executable, script, "with"] + opt + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        hists[name] = json.load(open(d / "train" / "train_summary.json"))
        res[name] = torch.load(d / "weights" / "agent.pt")
        if name != "uniform":
            assert "per_beta: " in r.stdout and "per_max_priority: " in r.stdout
    h = hists["per"][0]
    assert h["updates"] > 0 and 0.4 < h["per_beta"] <= 1.0 and h["per_max_priority"] >= 1.0
    assert "per_beta" not in hists["uniform"][0]
    assert hists["per"] == hists["per2"]
    assert all(torch.equal(res["per"][k], res["per2"][k]) for k in res["per"])
    assert any(not torch.equal(res["per"][k], res["uniform"][k]) for k in res["per"])


def test_train_agent_refuses_prioritized_replay_under_forced_dist(tmp_path):
    script = os.path.join(ROOT, "train_agent.py")
    env = dict(os.environ, PYTHONPATH=ROOT, IVOSW_FORCE_DIST="1")
    r = subprocess.run([sys.executable, script, "with", "agent.replay=prioritized", "synthetic=1", f"agent.save_result_dir={tmp_path}/t",
                        f"ckpt_dir={tmp_path}/w"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "one GPU only" in (r.stdout + r.stderr)
