"""GPU: the opt-in poly learning-rate schedule of the Double-DQN update (cfg.agent.lr_schedule = "poly", lr_pow, lr_total_steps) through
every path that carries an update, for both optimizers: the eager steps (ivosw_clamp_adam / ivosw_clamp_sgd fed the host table's lr), the
scheduled device entries (ivosw_clamp_{adam,sgd}_dev_sched), the one-call steps (ivosw_dqn_step_drawn[_sgd]_sched), CapturedDqnStep and the
loops built on it, the episode's device update loop, the data-parallel step on the backend collective and on the P2P all-reduce, and
train_agent.py.  The yardsticks: torch.optim.SGD on the CPU and the eager constant-lr Adam entry fed lr_k, the numpy oracle of clamp +
Adam, torch's own PolynomialLR, and the eager per-step updates (bit for bit)."""
import contextlib
import io
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ivos_w_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
SHAPES = [(128, 25), (32, 9)]


class AD(dict):
    __getattr__ = dict.__getitem__


def cfg(update_rate=0.5, lr=LR, weight_decay=5e-4, **opt):
    return AD(phase="train", data=AD(subset="train"),
              agent=AD(memory_size=1000, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500, update_rate=update_rate, lr=lr,
                       weight_decay=weight_decay, **opt))


def poly(n, lr_pow=0.9, optimizer="adam", **kw):
    opt = dict(optimizer="sgd", momentum=0.9, nesterov=kw.pop("nesterov", False)) if optimizer == "sgd" else {}
    return cfg(lr_schedule="poly", lr_pow=lr_pow, lr_total_steps=n, **opt, **kw)


def lr_k(k, n, lr=LR, lr_pow=0.9):
    return float(np.float32(lr * (1.0 - min(k, n) / n) ** lr_pow))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def load_brain(net, seed):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(seed).items()})


def make_agent(dev, c):
    from ivos_w_amd.models.agent import Agent
    a = Agent(dev, c)
    load_brain(a.policy_net, 0)
    load_brain(a.target_net, 1)
    return a


def opt_state(a):
    """The optimizer's tensors: Adam's moments or SGD's buffer, and the device state (counters) when there is one."""
    s = a.optimizer.state
    out = [s[k] for k in ("exp_avg", "exp_avg_sq", "momentum_buffer") if k in s and s[k] is not None]
    return out + ([s["dev"]] if s.get("dev") is not None else [])


def dev_counter(a):
    """The optimizer's device step counter (Adam: int32 at byte 16; SGD: int32 at byte 0)."""
    off = 16 if a.optimizer.kind == "adam" else 0
    return int(a.optimizer.state["dev"][off:off + 4].cpu().numpy().view(np.int32)[0])


def assert_same(x, y, what):
    assert torch.equal(x.policy_net.flat, y.policy_net.flat), what
    for u, v in zip(opt_state(x), opt_state(y)):
        assert torch.equal(u, v), what


# ------------------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("nesterov", [False, True])
def test_poly_sgd_matches_torch_optim_sgd(dev, B, T, nesterov):
    """12 steps with N = 8 (lr 0 from step 8 on), through the scheduled device entry (ivosw_clamp_sgd_dev_sched): torch.optim.SGD on the
    CPU, fed the GPU's own clamped gradients with group["lr"] = lr_k before each step, equal bit for bit."""
    tr = synth.replay_transitions(n=500, T=T, seed=11)
    agent = make_agent(dev, poly(8, optimizer="sgd", nesterov=nesterov))
    opt = agent.optimizer
    assert opt.kind == "sgd" and opt.scheduled
    p = torch.nn.Parameter(agent.policy_net.flat.detach().cpu().clone())
    ref = torch.optim.SGD([p], lr=LR, momentum=0.9, dampening=0, weight_decay=5e-4, nesterov=nesterov, foreach=False)
    opt.dev_state()
    for s in range(12):
        batch = synth.collate_np(tr, synth.minibatch_indices(s, n=500, B=B, seed=7))
        agent.loss_and_grads(batch)
        g = agent.policy_net.flat_grad.detach().cpu().clone()
        assert opt.current_lr() == lr_k(s, 8)
        opt.enqueue_dev_step()
        opt.note_dev_steps(1)
        ref.param_groups[0]["lr"] = lr_k(s, 8)
        p.grad = g.clamp(-1.0, 1.0)
        ref.step()
        np.testing.assert_array_equal(agent.policy_net.flat.cpu().numpy(), p.detach().numpy(), err_msg=f"step {s}")
        np.testing.assert_array_equal(opt.state["momentum_buffer"].cpu().numpy(), ref.state[p]["momentum_buffer"].numpy(), err_msg=f"step {s}")
        assert dev_counter(agent) == s + 1
    assert opt.current_lr() == 0.0


@pytest.mark.parametrize("B,T", SHAPES)
def test_poly_adam_is_the_constant_entry_fed_lr_k_and_matches_the_oracle(dev, B, T):
    """12 steps with N = 8 through ivosw_clamp_adam_dev_sched against ivosw_clamp_adam (the eager constant-lr entry) fed lr_k step by step,
    bit for bit; and every step against oracle.brain_oracle.clamp_adam(lr = lr_k) from the same state, within test_gpu_agent.py's
    tolerance on the parameter deltas."""
    from ivos_w_amd import _lib as L
    from oracle import brain_oracle as bo
    tr = synth.replay_transitions(n=500, T=T, seed=11)
    a, b = make_agent(dev, poly(8)), make_agent(dev, cfg())
    a.optimizer.dev_state()
    b.optimizer._ensure()
    offs = synth.brain_offsets()

    def as_dict(flat):
        return {k: flat[off:off + int(np.prod(shp))].copy() for k, (off, shp) in offs.items()}
    for s in range(12):
        batch = synth.collate_np(tr, synth.minibatch_indices(s, n=500, B=B, seed=7))
        a.loss_and_grads(batch)
        b.loss_and_grads(batch)
        P, M, V = (as_dict(t.cpu().numpy()) for t in (a.policy_net.flat, a.optimizer.state["exp_avg"], a.optimizer.state["exp_avg_sq"]))
        G = as_dict(a.policy_net.flat_grad.cpu().numpy())
        p0 = a.policy_net.flat.cpu().numpy().astype(np.float64)
        a.optimizer.enqueue_dev_step()
        a.optimizer.note_dev_steps(1)
        ob = b.optimizer
        L.check(L.lib().ivosw_clamp_adam(L.dptr(b.policy_net.flat), L.dptr(b.policy_net.flat_grad), L.dptr(ob.state["exp_avg"]),
                                         L.dptr(ob.state["exp_avg_sq"]), L.BRAIN_NPARAMS, s + 1, lr_k(s, 8), 0.9, 0.999, 1e-8, 5e-4, 1.0, 1.0,
                                         L.stream_ptr(dev)), "clamp_adam")
        assert torch.equal(a.policy_net.flat, b.policy_net.flat), s
        assert torch.equal(a.optimizer.state["exp_avg"], ob.state["exp_avg"]) and torch.equal(a.optimizer.state["exp_avg_sq"], ob.state["exp_avg_sq"])
        bo.clamp_adam(P, G, M, V, s + 1, lr_k(s, 8), 5e-4)
        got = a.policy_net.flat.cpu().numpy().astype(np.float64) - p0
        ulp = np.spacing(np.abs(p0).astype(np.float32)).astype(np.float64)
        for k, (off, shp) in offs.items():
            sl = slice(off, off + int(np.prod(shp)))
            want = P[k].astype(np.float64) - p0[sl]
            err = np.abs(got[sl] - want) - (5e-3 * np.abs(want) + 2e-8 + ulp[sl])
            assert err.max() <= 0, (s, k, err.max())
    assert dev_counter(a) == 12
    final = a.policy_net.flat.clone()
    a.loss_and_grads(synth.collate_np(tr, synth.minibatch_indices(12, n=500, B=B, seed=7)))
    a.optimizer.enqueue_dev_step()
    assert torch.equal(a.policy_net.flat, final)                      # lr 0 past N: the parameters stay, the moments move


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_against_torch_polynomial_lr(dev, optimizer):
    """A constant-lr run whose lr torch.optim.lr_scheduler.PolynomialLR sets before every step (its chained form, stepped after each
    optimizer step) against the poly run: parameters within 1e-6 relative (the chained form drifts from the closed form by float64 ulps)."""
    tr = synth.replay_transitions(n=500, T=25, seed=11)
    sched_agent = make_agent(dev, poly(8, lr_pow=0.9, optimizer=optimizer))
    plain = make_agent(dev, cfg(optimizer="sgd", momentum=0.9) if optimizer == "sgd" else cfg())
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR)
    sch = torch.optim.lr_scheduler.PolynomialLR(dummy, total_iters=8, power=0.9)
    for s in range(12):
        batch = synth.collate_np(tr, synth.minibatch_indices(s, n=500, B=128, seed=7))
        sched_agent.loss_and_grads(batch)
        sched_agent.optimizer.step()
        plain.loss_and_grads(batch)
        plain.optimizer.param_groups[0]["lr"] = dummy.param_groups[0]["lr"]
        plain.optimizer.step()
        dummy.step()
        sch.step()
        np.testing.assert_allclose(sched_agent.policy_net.flat.cpu().numpy(), plain.policy_net.flat.cpu().numpy(), rtol=1e-6, atol=0,
                                   err_msg=f"step {s}")


# ------------------------------------------------------------------------------------------------------------------- the device paths
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_one_call_step_equals_the_three_calls(dev, optimizer):
    """ivosw_dqn_step_drawn[_sgd]_sched (8 kernel nodes) against the un-folded sequence (DQN_ONECALL=0: 10 nodes) across N: the minibatch,
    loss, gradient arena, parameters, moments or buffer, and both device counters (draw, optimizer) bit for bit."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    seed = 0xABCDEF0123

    def build(onecall):
        L.tune_set(b"DQN_ONECALL", onecall)
        a = make_agent(dev, poly(4, optimizer=optimizer, nesterov=optimizer == "sgd"))
        return a, CapturedDqnStep(a, rp, 128, fused=True, draw_seed=seed)
    try:
        (a1, s1), (a0, s0) = build(1), build(0)
    finally:
        L.tune_set(b"DQN_ONECALL", 1)
    assert s1._onecall_entry == ("ivosw_dqn_step_drawn_sgd_sched" if optimizer == "sgd" else "ivosw_dqn_step_drawn_sched")
    assert (s1.kernel_nodes, s0.kernel_nodes) == (8, 10), (s1.kernel_nodes, s0.kernel_nodes)
    for c in range(7):
        s1.launch()
        s0.launch()
        for name in ("idx", "state", "new_state", "action", "r_step", "r_done", "loss"):
            assert torch.equal(getattr(s1, name), getattr(s0, name)), (c, name)
        assert torch.equal(a1.policy_net.flat_grad, a0.policy_net.flat_grad), c
        assert_same(a1, a0, c)
        assert torch.equal(s1.draw, s0.draw)
        assert dev_counter(a1) == dev_counter(a0) == c + 1
    assert a1.optimizer.state["step"] == a0.optimizer.state["step"] == 7


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_captured_and_multi_step_graphs_equal_eager_steps_across_n(dev, optimizer):
    """CapturedDqnStep (fused, rows written by the caller) and a steps=4 multi-step graph against eager per-step updates, 12 steps with N = 6:
    bit for bit at every step, and the parameters stop moving once lr reaches 0 (a graph with a baked lr cannot do that)."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay, draw_indices
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=2019), dev)
    B, N, seed = 128, 6, 77
    c = poly(N, optimizer=optimizer)
    eager, cap, multi = make_agent(dev, c), make_agent(dev, c), make_agent(dev, c)
    step = CapturedDqnStep(cap, rp, B, fused=True)
    four = CapturedDqnStep(multi, rp, B, fused=True, draw_seed=seed, steps=4)
    assert step.graph is not None and four.graph is not None
    at_n = None
    for s in range(12):
        idx = torch.from_numpy(draw_indices(seed, s, B, len(rp))).to(dev)
        l0 = eager.loss_and_grads(rp.sample(idx)).clone()
        eager.optimizer.step()
        step.idx.copy_(idx)
        l1 = step.launch().clone()
        assert torch.equal(l0, l1), s
        assert torch.equal(eager.policy_net.flat, cap.policy_net.flat), s
        for u, v in zip(opt_state(eager), opt_state(cap)[:len(opt_state(eager))]):
            assert torch.equal(u, v), s
        if s % 4 == 3:
            four.launch()
            assert torch.equal(eager.policy_net.flat, multi.policy_net.flat), s
        if s == N - 1:
            at_n = eager.policy_net.flat.clone()
    assert eager.optimizer.state["step"] == cap.optimizer.state["step"] == multi.optimizer.state["step"] == 12
    assert dev_counter(cap) == dev_counter(multi) == 12
    assert cap.optimizer.current_lr() == 0.0
    assert torch.equal(cap.policy_net.flat, at_n) and torch.equal(multi.policy_net.flat, at_n)
    assert not torch.equal(at_n, torch.from_numpy(synth.brain_flat(synth.brain_state_dict(0))).to(dev))


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_loops_and_device_update_loop_equal_per_step_update_agent(dev, capsys, monkeypatch, optimizer):
    """GraphedDqnLoop, LeanDqnLoop and AutoDqnLoop against update_agent per step on the same drawn minibatches and coins, 61 steps with
    N = 40; and the episode's device update loop (utils_agent._device_update_loop, train_agent.py's path) against its per-batch form: the
    host table and the device table give the same lr at every step."""
    from torch.utils.data import DataLoader
    from ivos_w_amd.datasets.agent_dataset import DAVIS2017AgentTrain
    from ivos_w_amd.models.agent import AutoDqnLoop, GraphedDqnLoop, LeanDqnLoop
    from ivos_w_amd.models.momory_pool import DeviceReplay, draw_indices
    from ivos_w_amd.utils import utils_agent
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    B, seed, n = 64, 99, 61
    c = poly(40, optimizer=optimizer, update_rate=0.05)
    ref = make_agent(dev, c)
    np.random.seed(5)
    for k in range(n):
        ref.update_agent(rp.sample(torch.from_numpy(draw_indices(seed, k, B, len(rp))).to(dev)))
    syncs = capsys.readouterr().out.count("target_net updated!")
    last = ref.loss[(ref.loss_position - 1) % ref.loss_capacity]
    for make, steps in ((lambda a: GraphedDqnLoop(a, rp, B, draw_seed=seed, block=8), (40, n - 40)),
                        (lambda a: LeanDqnLoop(a, rp, B, draw_seed=seed), (n,)),
                        (lambda a: AutoDqnLoop(a, rp, B, draw_seed=seed, block=8, probe=8), (33, n - 33))):
        other = make_agent(dev, c)
        np.random.seed(5)
        lp = make(other)
        loss = None
        for k in steps:
            loss = lp.run(k)
        capsys.readouterr()
        name = type(lp).__name__
        assert lp.syncs == syncs and other.optimizer.state["step"] == n, name
        assert torch.equal(other.policy_net.flat, ref.policy_net.flat), name
        assert torch.equal(other.target_net.flat, ref.target_net.flat), name
        for u, v in zip(opt_state(ref), opt_state(other)):
            assert torch.equal(u, v), name
        assert float(loss.item()) == last, name
    # the episode's update loop: device path against the per-batch path, two episodes of 10 steps, N = 15
    ds = DAVIS2017AgentTrain.from_soa(synth.replay_transitions(n=300, T=25, seed=3))
    out = {}
    for path in ("host", "device"):
        monkeypatch.setenv("IVOSW_UPDATE_PATH", "host" if path == "host" else "")
        torch.manual_seed(123)
        np.random.seed(5)
        agent = make_agent(dev, poly(15, optimizer=optimizer, update_rate=0.3))
        for episode in range(2):
            loader = DataLoader(ds, batch_size=32, shuffle=True, num_workers=0)
            got = utils_agent._device_update_loop(agent, loader, 14)
            if path == "host":
                assert got is None
                for i, sample in enumerate(loader):
                    if i == 14:
                        break
                    agent.update_agent(sample)
        out[path] = agent
    capsys.readouterr()
    assert out["host"].optimizer.state["step"] == out["device"].optimizer.state["step"] == 20
    assert torch.equal(out["host"].policy_net.flat, out["device"].policy_net.flat)
    assert torch.equal(out["host"].target_net.flat, out["device"].target_net.flat)
    for u, v in zip(opt_state(out["host"]), opt_state(out["device"])):
        assert torch.equal(u, v)


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_resume_and_eager_steps_between_captured_launches(dev, optimizer):
    """5 captured steps, state_dict, a fresh agent, load_state_dict, 5 more = 10 straight steps, bit for bit (the device counter resumes at
    k = 5, the lr at lr_5); and an eager step between captured launches resyncs the device counter."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay, draw_indices
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=2019), dev)
    B, N = 64, 7
    c = poly(N, optimizer=optimizer)
    idxs = [torch.from_numpy(draw_indices(3, s, B, len(rp))).to(dev) for s in range(10)]

    def run(agent, step, ks):
        for k in ks:
            step.idx.copy_(idxs[k])
            step.launch()
    straight = make_agent(dev, c)
    run(straight, CapturedDqnStep(straight, rp, B, fused=True), range(10))
    first = make_agent(dev, c)
    run(first, CapturedDqnStep(first, rp, B, fused=True), range(5))
    sd = first.optimizer.state_dict()
    assert (sd["param_groups"][0]["lr_schedule"], sd["param_groups"][0]["lr_total_steps"]) == ("poly", N)
    flat = first.policy_net.flat.clone()
    fresh = make_agent(dev, c)
    fresh.policy_net.flat.copy_(flat)
    fresh.optimizer.load_state_dict(sd)
    assert fresh.optimizer.current_lr() == lr_k(5, N)
    run(fresh, CapturedDqnStep(fresh, rp, B, fused=True), range(5, 10))
    assert dev_counter(fresh) == dev_counter(straight) == 10
    assert_same(fresh, straight, "resume")
    # captured, eager, captured, eager, captured: against 5 eager steps
    mixed, eager = make_agent(dev, c), make_agent(dev, c)
    step = CapturedDqnStep(mixed, rp, B, fused=True)
    for k in range(5):
        eager.loss_and_grads(rp.sample(idxs[k]))
        eager.optimizer.step()
        if k % 2 == 0:
            run(mixed, step, [k])
        else:
            mixed.loss_and_grads(rp.sample(idxs[k]))
            mixed.optimizer.step()
        assert torch.equal(mixed.policy_net.flat, eager.policy_net.flat), k
    assert dev_counter(mixed) == 5 and mixed.optimizer.state["step"] == 5


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_poly_changes_after_capture_are_refused_and_bad_options_touch_nothing(dev, optimizer):
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import Agent, CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=1000, T=25, seed=11), dev)
    a = make_agent(dev, poly(8, optimizer=optimizer))
    step = CapturedDqnStep(a, rp, 64, fused=True, draw_seed=5)
    step.launch()
    g = a.optimizer.param_groups[0]
    for key, value in (("lr_schedule", "constant"), ("lr", 2e-3), ("lr_pow", 1.0), ("lr_total_steps", 9)):
        old = g[key]
        g[key] = value
        with pytest.raises(RuntimeError, match="lr schedule"):
            step.launch()
        g[key] = old
    step.launch()
    # a refused entry call and a refused option leave the parameters, the optimizer state and the draw counter as they were
    torch.cuda.synchronize(dev)
    draw1, flat1, st1 = step.draw.clone(), a.policy_net.flat.clone(), [t.clone() for t in opt_state(a)]
    args = list(step._onecall_args)
    lib = L.lib()
    fn = getattr(lib, step._onecall_entry)
    at = 28 if optimizer == "sgd" else 29                               # lr_table
    for i, bad in ((at, None), (at + 1, 0), (at + 1, -3)):
        trial = list(args)
        trial[i] = bad
        assert fn(*trial, L.stream_ptr(dev)) == -1, (i, bad)
        assert step._onecall_entry in lib.ivosw_last_error().decode()
    g["lr_schedule"] = "Poly"
    with pytest.raises(ValueError):
        step.launch()
    with pytest.raises(ValueError):
        a.optimizer.step()
    g["lr_schedule"] = "poly"
    torch.cuda.synchronize(dev)
    assert torch.equal(step.draw, draw1) and torch.equal(a.policy_net.flat, flat1)
    for u, v in zip(opt_state(a), st1):
        assert torch.equal(u, v)
    for bad in (dict(lr_schedule="cosine"), dict(lr_schedule="poly"), dict(lr_schedule="poly", lr_total_steps=8, lr_pow=-1.0)):
        with pytest.raises(ValueError):
            Agent(dev, cfg(**bad))


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_constant_schedule_is_the_default_bit_for_bit(dev, optimizer):
    """lr_schedule="constant" (and lr_pow / lr_total_steps next to it) gives the bits of a config without the keys, on the one-call step
    with the unchanged node counts (8, and 10 off the fused chain) and on the eager step; no device table, no SGD counter."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    extra = dict(optimizer="sgd", momentum=0.9) if optimizer == "sgd" else {}
    agents = {}
    for onecall in (1, 0):
        for name, c in (("none", cfg(**extra)), ("constant", cfg(lr_schedule="constant", lr_pow=0.9, lr_total_steps=0, **extra))):
            L.tune_set(b"DQN_ONECALL", onecall)
            try:
                a = make_agent(dev, c)
                st = CapturedDqnStep(a, rp, 128, fused=True, draw_seed=21)
            finally:
                L.tune_set(b"DQN_ONECALL", 1)
            assert not a.optimizer.scheduled and st.kernel_nodes == (8 if onecall else 10), (name, st.kernel_nodes)
            assert st._onecall_entry == ("ivosw_dqn_step_drawn_sgd" if optimizer == "sgd" else "ivosw_dqn_step_drawn_ex")
            for _ in range(3):
                st.launch()
            a.loss_and_grads(rp.sample(st.idx))
            a.optimizer.step()
            assert "dev" not in a.optimizer.state or optimizer == "adam"
            agents[(onecall, name)] = a
    for onecall in (1, 0):
        assert_same(agents[(onecall, "none")], agents[(onecall, "constant")], onecall)
    assert torch.equal(agents[(1, "none")].policy_net.flat, agents[(0, "none")].policy_net.flat)


# ------------------------------------------------------------------------------------------------------------------- data parallel
DP_STEPS, DP_B, DP_N = 3, 128, 2


def _batch(tr, idx):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.collate_np(tr, idx).items()}


def _collect(procs, q, n, timeout=600):
    """n results from the workers' queue.  Fails as soon as a worker reports an error or ends without a result, and never leaves a worker
    behind: a rank whose peer died may wait in a collective forever, so whatever is still running at the end is killed."""
    import queue
    import time
    out, t0 = [], time.time()
    try:
        while len(out) < n:
            try:
                item = q.get(timeout=2)
            except queue.Empty:
                ended = [p.exitcode for p in procs if p.exitcode is not None]
                assert not any(e != 0 for e in ended), f"a worker ended without a result (exit codes {[p.exitcode for p in procs]})"
                assert len(ended) < len(procs), "every worker ended without sending its result"
                assert time.time() - t0 < timeout, f"no result from the workers within {timeout} s"
                continue
            assert not (isinstance(item, tuple) and len(item) == 2 and item[0] == "error"), item[1] if isinstance(item, tuple) else item
            out.append(item)
        for p in procs:
            p.join(120)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return out


def _dp_worker(rank, world, port, q, mode, optimizer):
    from ivos_w_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      IVOSW_P2P="0" if mode == "backend" else "1")
    r, w, dev = parallel.init("gloo")
    assert dev.type == "cuda" and w == 2
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, poly(DP_N, optimizer=optimizer))
    np.random.seed(5)
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(DP_STEPS):
            idx = synth.minibatch_indices(s, n=2000, B=DP_B, seed=7)
            agent.update_agent(_batch(tr, idx[rank * (DP_B // 2):(rank + 1) * (DP_B // 2)]))
            out.append((agent.policy_net.flat.cpu().numpy().copy(), agent.target_net.flat.cpu().numpy().copy()))
    assert parallel.collective_path(agent.policy_net.flat_grad) == mode
    q.put((rank, out))
    for v in parallel._P2P.values():
        if v is not None:
            v.close()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _run_dp_worker(*args):
    try:
        _dp_worker(*args)
    except BaseException:
        import traceback
        args[3].put(("error", traceback.format_exc()))
        raise


def _free_port():
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    return port


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("mode", ["backend", "p2p"])
def test_poly_world2_matches_single_process_full_batch(mode, optimizer):
    """Two ranks of half the batch each, N = 2 (the third step runs at lr 0): replicas bit-identical after every step, the parameters close
    to the single-process full batch's, and unmoved by the lr-0 step."""
    from ivos_w_amd.models.agent import lr_schedule_option  # noqa: F401  (without the feature: fail here, before any worker starts)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_dp_worker, args=(r, 2, port, q, mode, optimizer)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(_collect(procs, q, 2))
    for a, b in zip(res[0], res[1]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(res[0][DP_N][0], res[0][DP_N - 1][0])      # lr 0 from step N on
    dev = torch.device("cuda:0")
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, poly(DP_N, optimizer=optimizer))
    start = agent.policy_net.flat.cpu().numpy().copy()
    np.random.seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(DP_STEPS):
            agent.update_agent(_batch(tr, synth.minibatch_indices(s, n=2000, B=DP_B, seed=7)))
    d1 = agent.policy_net.flat.cpu().numpy().astype(np.float64) - start
    d2 = res[0][-1][0].astype(np.float64) - start
    assert np.abs(d1).max() > 0.1 * LR                  # the steps moved the parameters
    if optimizer == "adam":                             # the tolerances of test_gpu_dist.py (Adam) and test_gpu_dqn_sgd.py (SGD)
        close = np.abs(d2 - d1) <= 1e-2 * np.abs(d1) + 0.05 * LR * DP_STEPS
    else:
        close = np.abs(d2 - d1) <= 1e-2 * np.abs(d1) + 1e-3 * np.abs(d1).max() + 2 * np.spacing(np.abs(start))
    assert close.mean() > 0.999, close.mean()


def _rccl_world1_worker(port, q, forced):
    from ivos_w_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      IVOSW_FORCE_DIST="1" if forced else "0", IVOSW_P2P="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r, w, dev = parallel.init("nccl")
    assert w == 1
    if forced:
        assert torch.distributed.is_initialized() and parallel.collective_active()
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    out = []
    for optimizer in ("adam", "sgd"):
        agent = make_agent(dev, poly(2, optimizer=optimizer))
        np.random.seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            for s in range(3):
                agent.update_agent(_batch(tr, synth.minibatch_indices(s, n=2000, B=128, seed=7)))
                out.append((agent.policy_net.flat.cpu().numpy().copy(), *(t.cpu().numpy().copy() for t in opt_state(agent))))
    q.put(out)
    if forced:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def _run_rccl_world1_worker(port, q, forced):
    try:
        _rccl_world1_worker(port, q, forced)
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))
        raise


def test_poly_rccl_world1_steps_are_bit_identical_to_the_single_process_steps():
    from ivos_w_amd.models.agent import lr_schedule_option  # noqa: F401  (without the feature: fail here, before any worker starts)
    ctx = mp.get_context("spawn")
    got = {}
    for forced in (True, False):
        q = ctx.Queue()
        p = ctx.Process(target=_run_rccl_world1_worker, args=(_free_port(), q, forced))
        p.start()
        got[forced] = _collect([p], q, 1)[0]
    for a, b in zip(got[True], got[False]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------- train_agent.py
def test_train_agent_with_poly(tmp_path):
    """train_agent.py with agent.lr_schedule=poly completes on the synthetic session; its checkpoint differs from the constant-lr run's, and
    the lr train_summary.json reports per epoch is lr_k at that epoch's update count (the constant run reports the base lr)."""
    from ivos_w_amd.models.agent import poly_lr_table
    script = os.path.join(ROOT, "train_agent.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    res, hists = {}, {}
    N = 20
    for name, opt in (("poly", ["agent.lr_schedule=poly", f"agent.lr_total_steps={N}", "agent.lr=1e-4"]), ("constant", ["agent.lr=1e-4"])):
        d = tmp_path / name
        common = ["synthetic=1", "synth.n_sequences=2", "synth.n_frames=26", "synth.height=120", "synth.width=216", f"ckpt_dir={d}/weights",
                  f"report_save_dir={d}/results", f"agent.save_result_dir={d}/train", "num_epochs=2", "agent.train_batch_size=16"]
        r = subprocess.run([sys.executable, script, "with"] + opt + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        hists[name] = json.load(open(d / "train" / "train_summary.json"))
        res[name] = torch.load(d / "weights" / "agent.pt")
        assert "lr: " in r.stdout
    table = poly_lr_table(1e-4, 0.9, N)
    for h in hists["poly"]:
        assert h["updates"] > 0 and h["lr"] == float(table[min(h["updates"], N)]), h
    assert hists["poly"][-1]["lr"] < 1e-4
    assert all(h["lr"] == 1e-4 for h in hists["constant"])
    assert [h["updates"] for h in hists["poly"]] == [h["updates"] for h in hists["constant"]]
    assert any(not torch.equal(res["poly"][k], res["constant"][k]) for k in res["poly"])
