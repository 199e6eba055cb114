"""GPU: the opt-in clamp + SGD update of the Double-DQN step (cfg.agent.optimizer = "sgd", momentum, nesterov) through every path that
carries an update: eager FusedClampSGD.step (ivosw_clamp_sgd), the one-call step (ivosw_dqn_step_drawn_sgd), CapturedDqnStep and the three
loops built on it, the data-parallel step on the backend collective and on the P2P all-reduce (ivosw_p2p_allreduce_clamp_sgd), RCCL with a
world of one, and train_agent.py.  The yardsticks: torch.optim.SGD on the CPU fed the GPU's own clamped gradients (bit for bit), an fp64
step built on oracle/brain_oracle.py, and the un-folded or eager sequences (bit for bit)."""
import io
import contextlib
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


def sgd_cfg(momentum=0.9, nesterov=False, **kw):
    return cfg(optimizer="sgd", momentum=momentum, nesterov=nesterov, **kw)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def load_brain(net, seed):
    sd = synth.brain_state_dict(seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd


def make_agent(dev, c):
    from ivos_w_amd.models.agent import Agent
    a = Agent(dev, c)
    load_brain(a.policy_net, 0)
    load_brain(a.target_net, 1)
    return a


COMBOS = [(0.0, False, 0.0), (0.0, False, 5e-4), (0.9, False, 0.0), (0.9, False, 5e-4), (0.9, True, 0.0), (0.9, True, 5e-4)]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("momentum,nesterov,wd", COMBOS)
def test_sgd_matches_torch_optim_sgd_on_the_gpus_gradients(dev, B, T, momentum, nesterov, wd):
    """6 steps; torch.optim.SGD on the CPU gets exactly the gradients the GPU produced, clamped on the host: parameters and momentum
    buffers equal (assert_array_equal: +0 == -0, the one difference the zero-initialised buffer allows)."""
    from ivos_w_amd.models.agent import FusedClampSGD
    tr = synth.replay_transitions(n=500, T=T, seed=11)
    agent = make_agent(dev, sgd_cfg(momentum=momentum, nesterov=nesterov, weight_decay=wd))
    assert isinstance(agent.optimizer, FusedClampSGD) and agent.optimizer.kind == "sgd"
    p = torch.nn.Parameter(agent.policy_net.flat.detach().cpu().clone())
    ref = torch.optim.SGD([p], lr=LR, momentum=momentum, dampening=0, weight_decay=wd, nesterov=nesterov, foreach=False)
    for s in range(6):
        batch = synth.collate_np(tr, synth.minibatch_indices(s, n=500, B=B, seed=7))
        agent.loss_and_grads(batch)
        g = agent.policy_net.flat_grad.detach().cpu().clone()
        agent.optimizer.step()
        p.grad = g.clamp(-1.0, 1.0)
        ref.step()
        np.testing.assert_array_equal(agent.policy_net.flat.cpu().numpy(), p.detach().numpy(), err_msg=f"step {s}")
        if momentum > 0:
            np.testing.assert_array_equal(agent.optimizer.state["momentum_buffer"].cpu().numpy(), ref.state[p]["momentum_buffer"].numpy(),
                                          err_msg=f"step {s}")
    assert agent.optimizer.state["step"] == 6
    assert not np.array_equal(agent.policy_net.flat.cpu().numpy(), synth.brain_flat(synth.brain_state_dict(0)))


@pytest.mark.parametrize("B,T", SHAPES)
def test_sgd_step_vs_fp64_oracle(dev, B, T):
    """Loss and gradient of the oracle's BPTT in fp64, then an fp64 clamp + SGD step (first step: buffer = d): the parameter deltas within
    the tolerances test_gpu_agent.py uses for Adam's (rtol 5e-3, atol 2e-8), plus one fp32 ulp of the parameter (most SGD deltas are
    smaller than that: the stored parameter cannot resolve them)."""
    from oracle import brain_oracle as bo
    tr = synth.replay_transitions(n=500, T=T, seed=11)
    agent = make_agent(dev, sgd_cfg(momentum=0.9, nesterov=True))
    P, Pt = synth.brain_state_dict(0), synth.brain_state_dict(1)
    batch = synth.collate_np(tr, synth.minibatch_indices(0, n=500, B=B, seed=7))
    p0 = synth.brain_flat(P).astype(np.float64)
    loss = float(agent.loss_and_grads(batch).item())
    agent.optimizer.step()
    ref_loss, G = bo.dqn_loss_and_grads(P, Pt, batch, 0.95)
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    g = np.clip(synth.brain_flat(G).astype(np.float64), -1.0, 1.0)
    d = g + 5e-4 * p0
    buf = d
    d = d + 0.9 * buf
    want = -LR * d
    got = agent.policy_net.flat.cpu().numpy().astype(np.float64) - p0
    ulp = np.spacing(np.abs(p0).astype(np.float32)).astype(np.float64)
    for k, (off, shp) in synth.brain_offsets().items():
        sl = slice(off, off + int(np.prod(shp)))
        err = np.abs(got[sl] - want[sl]) - (5e-3 * np.abs(want[sl]) + 2e-8 + ulp[sl])
        assert err.max() <= 0, (k, err.max())
    assert np.abs(got).max() > 0.5 * np.abs(want).max() > 0


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("B", [128, 32])
def test_sgd_one_call_step_equals_the_three_calls(dev, loss, B):
    """ivosw_dqn_step_drawn_sgd (8 kernel nodes) against ivosw_replay_draw_gather + ivosw_dqn_loss_grad_ex + ivosw_clamp_sgd
    (DQN_ONECALL=0: 10 nodes), 5 steps, bit for bit."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay, draw_indices
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    seed = 0xABCDEF0123
    extra = dict(loss="huber", huber_delta=0.1) if loss == "huber" else {}

    def build(onecall):
        L.tune_set(b"DQN_ONECALL", onecall)
        a = make_agent(dev, sgd_cfg(momentum=0.9, nesterov=True, **extra))
        return a, CapturedDqnStep(a, rp, B, fused=True, draw_seed=seed)
    try:
        (a1, s1), (a0, s0) = build(1), build(0)
    finally:
        L.tune_set(b"DQN_ONECALL", 1)
    assert s1._onecall_entry == "ivosw_dqn_step_drawn_sgd"
    assert (s1.kernel_nodes, s0.kernel_nodes) == (8, 10), (s1.kernel_nodes, s0.kernel_nodes)
    for c in range(5):
        s1.launch()
        s0.launch()
        np.testing.assert_array_equal(s1.idx.cpu().numpy(), draw_indices(seed, c, B, len(rp)))
        for name in ("idx", "state", "new_state", "action", "r_step", "r_done", "loss"):
            assert torch.equal(getattr(s1, name), getattr(s0, name)), (c, name)
        assert torch.equal(a1.policy_net.flat_grad, a0.policy_net.flat_grad), c
        assert torch.equal(a1.policy_net.flat, a0.policy_net.flat), c
        assert torch.equal(a1.optimizer.state["momentum_buffer"], a0.optimizer.state["momentum_buffer"]), c
        assert torch.equal(s1.draw, s0.draw)
    assert a1.optimizer.state["step"] == a0.optimizer.state["step"] == 5
    assert not torch.equal(a1.policy_net.flat, torch.from_numpy(synth.brain_flat(synth.brain_state_dict(0))).to(dev))


@pytest.mark.parametrize("fused", [True, False])
def test_sgd_captured_step_is_bit_identical_to_eager(dev, fused):
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=2019), dev)
    B = 128
    idxs = [torch.from_numpy(synth.minibatch_indices(s, n=3000, B=B, seed=7)).to(dev) for s in range(6)]
    c = sgd_cfg(momentum=0.9, nesterov=True)
    eager, cap = make_agent(dev, c), make_agent(dev, c)
    step = CapturedDqnStep(cap, rp, B, fused=fused)
    for s, idx in enumerate(idxs):
        l0 = eager.loss_and_grads(rp.sample(idx)).clone()
        g0 = eager.policy_net.flat_grad.clone()
        eager.optimizer.step()
        step.idx.copy_(idx)
        l1 = step.launch().clone()
        g1 = cap.policy_net.flat_grad.clone()
        if not fused:
            cap.optimizer.step()
        assert torch.equal(l0, l1) and torch.equal(g0, g1), s
        assert torch.equal(eager.policy_net.flat, cap.policy_net.flat), s
        assert torch.equal(eager.optimizer.state["momentum_buffer"], cap.optimizer.state["momentum_buffer"]), s
    assert eager.optimizer.state["step"] == cap.optimizer.state["step"] == 6
    if fused:       # the optimizer's values are baked into the graph: changing them afterwards is refused
        g = cap.optimizer.param_groups[0]
        for key, value in (("momentum", 0.5), ("nesterov", False), ("lr", 2e-3), ("weight_decay", 0.0)):
            old = g[key]
            g[key] = value
            with pytest.raises(RuntimeError, match="momentum / nesterov"):
                step.launch()
            g[key] = old
        step.launch()


def test_sgd_multi_step_graph_equals_single_steps(dev):
    """CapturedDqnStep(steps=4): four SGD steps per launch (nothing but the buffer and the draw counter carries over) = four launches."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    c = sgd_cfg(momentum=0.9)
    a1, a4 = make_agent(dev, c), make_agent(dev, c)
    one = CapturedDqnStep(a1, rp, 128, fused=True, draw_seed=77)
    four = CapturedDqnStep(a4, rp, 128, fused=True, draw_seed=77, steps=4)
    for _ in range(2):
        for _ in range(4):
            one.launch()
        four.launch()
    assert torch.equal(one.loss, four.loss) and torch.equal(one.draw, four.draw)
    assert torch.equal(a1.policy_net.flat, a4.policy_net.flat)
    assert torch.equal(a1.optimizer.state["momentum_buffer"], a4.optimizer.state["momentum_buffer"])
    assert a1.optimizer.state["step"] == a4.optimizer.state["step"] == 8


def test_sgd_loops_equal_per_step_update_agent(dev, capsys):
    """GraphedDqnLoop, LeanDqnLoop and AutoDqnLoop against update_agent per step on the same drawn minibatches (the host mirror of the
    device draw) and the same coin stream: parameters, target net, momentum buffer, syncs and the last loss bit for bit."""
    from ivos_w_amd.models.agent import AutoDqnLoop, GraphedDqnLoop, LeanDqnLoop
    from ivos_w_amd.models.momory_pool import DeviceReplay, draw_indices
    rp = DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=11), dev)
    B, seed, n = 64, 99, 61
    c = sgd_cfg(momentum=0.9, nesterov=True, update_rate=0.05)
    ref = make_agent(dev, c)
    np.random.seed(5)
    for k in range(n):
        idx = torch.from_numpy(draw_indices(seed, k, B, len(rp))).to(dev)
        ref.update_agent(rp.sample(idx))
    syncs = capsys.readouterr().out.count("target_net updated!")
    assert syncs > 0 and ref.optimizer.state["step"] == n
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
        assert lp.syncs == syncs and other.optimizer.state["step"] == n, type(lp).__name__
        assert torch.equal(other.policy_net.flat, ref.policy_net.flat), type(lp).__name__
        assert torch.equal(other.target_net.flat, ref.target_net.flat), type(lp).__name__
        assert torch.equal(other.optimizer.state["momentum_buffer"], ref.optimizer.state["momentum_buffer"]), type(lp).__name__
        assert float(loss.item()) == last, type(lp).__name__


def test_sgd_is_not_adam_and_bad_options_touch_nothing(dev):
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import Agent, CapturedDqnStep
    from ivos_w_amd.models.momory_pool import DeviceReplay
    rp = DeviceReplay(synth.replay_transitions(n=1000, T=25, seed=11), dev)
    flats = {}
    for name, c in (("adam", cfg(lr=LR)), ("sgd", sgd_cfg(momentum=0.9))):
        a = make_agent(dev, c)
        assert a.optimizer.kind == name
        step = CapturedDqnStep(a, rp, 64, fused=True, draw_seed=5)
        for _ in range(3):
            step.launch()
        flats[name] = a.policy_net.flat.cpu().numpy()
    assert not np.allclose(flats["adam"], flats["sgd"], rtol=1e-6, atol=0)
    # a refused option leaves the parameters, the buffer and the draw counter as they were
    a = make_agent(dev, sgd_cfg(momentum=0.9))
    step = CapturedDqnStep(a, rp, 16, fused=True, draw_seed=5, capture=False)
    step.launch()
    torch.cuda.synchronize(dev)
    draw1, flat1, buf1 = step.draw.clone(), a.policy_net.flat.clone(), a.optimizer.state["momentum_buffer"].clone()
    args = list(step._onecall_args)
    assert len(args) == 33
    lib = L.lib()
    for i, bad in ((27, -1e-3), (28, float("nan")), (29, -1.0), (30, 2), (28, 0.0)):
        trial = list(args)
        trial[i] = bad
        if i == 28 and bad == 0.0:
            trial[30] = 1                                     # nesterov without momentum
        assert lib.ivosw_dqn_step_drawn_sgd(*trial, L.stream_ptr(dev)) == -1, (i, bad)
        assert lib.ivosw_last_error().decode()
    assert lib.ivosw_clamp_sgd(L.dptr(a.policy_net.flat), L.dptr(a.policy_net.flat_grad), L.dptr(a.optimizer.state["momentum_buffer"]),
                               L.BRAIN_NPARAMS, -1.0, 0.9, 0.0, 0, 1.0, 1.0, L.stream_ptr(dev)) == -1
    torch.cuda.synchronize(dev)
    assert torch.equal(step.draw, draw1) and torch.equal(a.policy_net.flat, flat1)
    assert torch.equal(a.optimizer.state["momentum_buffer"], buf1)
    for bad in (dict(optimizer="rmsprop"), dict(optimizer="sgd", momentum=0.0, nesterov=True), dict(optimizer="sgd", momentum=-1.0)):
        with pytest.raises(ValueError):
            Agent(dev, cfg(**bad))
    # an Adam state dict is refused, an SGD one round-trips
    sd = a.optimizer.state_dict()
    with pytest.raises(ValueError):
        a.optimizer.load_state_dict(make_agent(dev, cfg()).optimizer.state_dict())
    a.optimizer.load_state_dict(sd)
    assert torch.equal(a.optimizer.state["momentum_buffer"], buf1)


# ------------------------------------------------------------------------------------------------------------------- data parallel
DP_STEPS, DP_B = 3, 128


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


def _dp_worker(rank, world, port, q, mode):
    from ivos_w_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      IVOSW_P2P="0" if mode == "backend" else "1")
    r, w, dev = parallel.init("gloo")
    assert dev.type == "cuda" and w == 2
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, sgd_cfg(momentum=0.9, nesterov=True))
    np.random.seed(5)
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(DP_STEPS):
            idx = synth.minibatch_indices(s, n=2000, B=DP_B, seed=7)
            agent.update_agent(_batch(tr, idx[rank * (DP_B // 2):(rank + 1) * (DP_B // 2)]))
            out.append((agent.policy_net.flat_grad.cpu().numpy().copy(), agent.policy_net.flat.cpu().numpy().copy(),
                        agent.target_net.flat.cpu().numpy().copy(), agent.optimizer.state["momentum_buffer"].cpu().numpy().copy()))
    path = parallel.collective_path(agent.policy_net.flat_grad)
    assert path == mode, (mode, path)
    q.put((rank, out))
    for v in parallel._P2P.values():
        if v is not None:
            v.close()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _run_dp_worker(rank, world, port, q, mode):
    try:
        _dp_worker(rank, world, port, q, mode)
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))
        raise


def _free_port():
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    return port


@pytest.mark.parametrize("mode", ["backend", "p2p"])
def test_sgd_world2_matches_single_process_full_batch(mode):
    from ivos_w_amd.models.agent import FusedClampSGD  # noqa: F401  (without the feature: fail here, before any worker starts)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_dp_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(_collect(procs, q, 2))
    for a, b in zip(res[0], res[1]):                    # replicas bit-identical after every step
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    dev = torch.device("cuda:0")
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, sgd_cfg(momentum=0.9, nesterov=True))
    start = agent.policy_net.flat.cpu().numpy().copy()
    np.random.seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(DP_STEPS):
            agent.update_agent(_batch(tr, synth.minibatch_indices(s, n=2000, B=DP_B, seed=7)))
            if s == 0:
                want = agent.policy_net.flat_grad.cpu().numpy()
                got = res[0][0][0] * 0.5                # the sum over ranks, scaled inside the update kernel
                np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-6 * np.abs(want).max())
    d1 = agent.policy_net.flat.cpu().numpy().astype(np.float64) - start
    d2 = res[0][-1][1].astype(np.float64) - start
    assert np.abs(d1).max() > 0.1 * LR                  # the steps moved the parameters
    close = np.abs(d2 - d1) <= 1e-2 * np.abs(d1) + 1e-3 * np.abs(d1).max() + 2 * np.spacing(np.abs(start))
    assert close.mean() > 0.999, close.mean()
    assert np.array_equal(res[0][-1][2], res[0][-1][1]) == bool(torch.equal(agent.target_net.flat, agent.policy_net.flat))


def _rccl_world1_worker(port, q, forced):
    from ivos_w_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      IVOSW_FORCE_DIST="1" if forced else "0", IVOSW_P2P="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r, w, dev = parallel.init("nccl")
    assert w == 1
    if forced:
        assert torch.distributed.is_initialized() and parallel.collective_active()
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, sgd_cfg(momentum=0.9))
    np.random.seed(5)
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(3):
            agent.update_agent(_batch(tr, synth.minibatch_indices(s, n=2000, B=128, seed=7)))
            out.append((agent.policy_net.flat_grad.cpu().numpy().copy(), agent.policy_net.flat.cpu().numpy().copy(),
                        agent.target_net.flat.cpu().numpy().copy(), agent.optimizer.state["momentum_buffer"].cpu().numpy().copy()))
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


def test_sgd_rccl_world1_steps_are_bit_identical_to_the_single_process_steps():
    from ivos_w_amd.models.agent import FusedClampSGD  # noqa: F401  (without the feature: fail here, before any worker starts)
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
    assert np.abs(got[True][0][0]).max() > 0


# ------------------------------------------------------------------------------------------------------------------- train_agent.py
_COUNTING_RUN = """
import runpy, sys
sys.path.insert(0, {root!r})
from ivos_w_amd.models import agent as A
count = [0]
apply = A.Agent.apply_gradients
def counted(self, *a, **k):
    count[0] += 1
    return apply(self, *a, **k)
A.Agent.apply_gradients = counted
sys.argv = [{script!r}] + sys.argv[1:]
runpy.run_path({script!r}, run_name="__main__")
print("STEPS_TAKEN", count[0])
"""


def test_train_agent_with_sgd(tmp_path):
    """train_agent.py with agent.optimizer=sgd agent.momentum=0.9 completes; train_summary.json's `updates` is the number of update steps
    taken, and the trained parameters differ from those of an Adam run with the same seed."""
    from ivos_w_amd.models.agent import FusedClampSGD  # noqa: F401  (without the feature: fail here, before two training runs)
    script = os.path.join(ROOT, "train_agent.py")
    runner = tmp_path / "run_counted.py"
    runner.write_text(_COUNTING_RUN.format(root=ROOT, script=script))
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = {}
    for name, opt in (("sgd", ["agent.optimizer=sgd", "agent.momentum=0.9"]), ("adam", [])):
        d = tmp_path / name
        common = ["synthetic=1", "synth.n_sequences=2", "synth.n_frames=26", "synth.height=120", "synth.width=216", f"ckpt_dir={d}/weights",
                  f"report_save_dir={d}/results", f"agent.save_result_dir={d}/train", "num_epochs=1", "agent.train_batch_size=16"]
        r = subprocess.run([sys.executable, str(runner), "with"] + opt + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        steps = int(r.stdout.rsplit("STEPS_TAKEN", 1)[1].split()[0])
        hist = json.load(open(d / "train" / "train_summary.json"))
        assert steps > 0 and hist[-1]["updates"] == steps, (name, steps, hist)
        res[name] = torch.load(d / "weights" / "agent.pt")
    assert any(not torch.equal(res["sgd"][k], res["adam"][k]) for k in res["sgd"])
