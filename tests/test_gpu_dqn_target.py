"""GPU: agent.target_update = "soft" | "periodic" (the target-network rule on the device) through every path that carries an update.
The yardsticks are code that existed before the option: the "coin" agent stepped with the single-step captured graph and an explicit
sync_target() (periodic) or a CPU torch lerp_ of the target (soft) after each step, and the host mirror target_update_mirror.  Every
equality is exact (torch.equal): the device fmaf is correctly rounded and everything else is the same entry points."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ivos_w_amd import synth

pytestmark = pytest.mark.gpu

LR = 1e-3


class AD(dict):
    __getattr__ = dict.__getitem__


OPTS = {"adam": dict(), "sgd": dict(optimizer="sgd", momentum=0.9, nesterov=True),
        "adam_poly": dict(lr_schedule="poly", lr_pow=0.9, lr_total_steps=40),
        "sgd_poly": dict(optimizer="sgd", momentum=0.9, lr_schedule="poly", lr_pow=0.9, lr_total_steps=40)}


def cfg(update_rate=0.5, **opt):
    return AD(phase="train", data=AD(subset="train"),
              agent=AD(memory_size=1000, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500, update_rate=update_rate, lr=LR,
                       weight_decay=5e-4, **opt))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def replay(dev):
    from ivos_w_amd.models.momory_pool import DeviceReplay
    return DeviceReplay(synth.replay_transitions(n=3000, T=25, seed=2019), dev)


def make_agent(dev, **opt):
    from ivos_w_amd.models.agent import Agent
    a = Agent(dev, cfg(**opt))
    for net, seed in ((a.policy_net, 0), (a.target_net, 1)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(seed).items()})
    return a


def tensors(a):
    """Everything a step changes: parameters, target, the optimizer's tensors and (when there is one) its device state."""
    s = a.optimizer.state
    out = [a.policy_net.flat, a.target_net.flat] + [s[k] for k in ("exp_avg", "exp_avg_sq", "momentum_buffer") if s.get(k) is not None]
    return out + ([s["dev"]] if s.get("dev") is not None else [])


def assert_same(x, y, what):
    tx, ty = tensors(x), tensors(y)
    assert len(tx) == len(ty), what
    for i, (u, v) in enumerate(zip(tx, ty)):
        assert torch.equal(u, v), (what, i)


def target_counter(a):
    return int(a._target_dev[0:4].cpu().numpy().view(np.int32)[0])


# ------------------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("n,offset", [(180993, 0), (1003, 0), (1003, 1), (7, 3)])
@pytest.mark.parametrize("mode", ["soft", "periodic"])
def test_target_update_alone_equals_the_host_mirror(dev, mode, n, offset):
    """ivosw_target_update against target_update_mirror, 9 launches on fresh policies: bit for bit after every launch, the counter advances by
    one per launch; `offset` moves the arenas off 16-byte alignment (the scalar form of the kernel), and the elements around them stay."""
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.agent import target_update_mirror
    assert n == L.BRAIN_NPARAMS or n < 2000
    lib = L.lib()
    rng = np.random.RandomState(n + offset)
    kw = dict(tau=0.05) if mode == "soft" else dict(period=4)
    args = (L.TARGET_SOFT, float(np.float32(0.05)), 0) if mode == "soft" else (L.TARGET_PERIODIC, 0.0, 4)
    host_t = rng.randn(n).astype(np.float32)
    buf_t = torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
    buf_p = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    t, p = buf_t[offset:offset + n], buf_p[offset:offset + n]
    t.copy_(torch.from_numpy(host_t))
    state = torch.zeros(lib.ivosw_target_state_bytes(), dtype=torch.uint8, device=dev)
    changed = 0
    for k in range(1, 10):
        host_p = (rng.randn(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        p.copy_(torch.from_numpy(host_p))
        L.check(lib.ivosw_target_update(L.dptr(t), L.dptr(p), n, *args, L.dptr(state), L.stream_ptr(dev)), "target_update")
        want = target_update_mirror(host_t, host_p, mode, k=k, **kw)
        changed += int((want != host_t).any())
        host_t = want
        np.testing.assert_array_equal(t.cpu().numpy().view(np.int32), want.view(np.int32), err_msg=f"launch {k}")
        got = state.cpu().numpy().view(np.int32)
        assert got[0] == k and got[1] == 0, (k, got)
    assert changed == (9 if mode == "soft" else 2)
    assert bool((buf_t[:offset] == 7.0).all()) and bool((buf_t[offset + n:] == 7.0).all())
    # a resumed counter: written by the caller, read by the next launch
    state[0:4].copy_(torch.from_numpy(np.array([3], dtype=np.int32).view(np.uint8)))
    L.check(lib.ivosw_target_update(L.dptr(t), L.dptr(p), n, *args, L.dptr(state), L.stream_ptr(dev)), "target_update")
    np.testing.assert_array_equal(t.cpu().numpy(), target_update_mirror(host_t, host_p, mode, k=4, **kw))
    assert state.cpu().numpy().view(np.int32)[0] == 4


# ------------------------------------------------------------------------------------------------------------------- against the coin agent
def coin_reference(dev, replay, B, seed, n, opt, after_step):
    """A "coin" agent (update_rate 0: the coin never fires) stepped n times with the single-step captured graph; after_step(agent, k) is
    called after step k = 1 .. n.  Returns the agent and the last loss."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    a = make_agent(dev, update_rate=0.0, **opt)
    step = CapturedDqnStep(a, replay, B, fused=True, draw_seed=seed)
    assert step.graph is not None and not step.tgt
    loss = None
    for k in range(1, n + 1):
        loss = step.launch()
        after_step(a, k)
    return a, loss.clone()


@pytest.mark.parametrize("opt", sorted(OPTS))
def test_periodic_graphed_loop_equals_coin_steps_with_explicit_syncs(dev, replay, opt):
    """period K = 5, GraphedDqnLoop with block 8 over 28 steps (three 8-step graphs and four single steps; syncs fall inside graphs) against
    the coin agent with sync_target() after every 5th step."""
    from ivos_w_amd.models.agent import GraphedDqnLoop
    B, seed, n, K = 64, 77, 28, 5
    ref, ref_loss = coin_reference(dev, replay, B, seed, n, OPTS[opt], lambda a, k: a.sync_target() if k % K == 0 else None)
    a = make_agent(dev, target_update="periodic", target_period=K, **OPTS[opt])
    before = np.random.get_state()
    loop = GraphedDqnLoop(a, replay, B, draw_seed=seed, block=8)
    assert loop.one.tgt and loop.many.tgt and loop.one._onecall_entry == "ivosw_dqn_step_drawn_tgt"
    loss = loop.run(24)
    loss = loop.run(4)
    after = np.random.get_state()
    assert loop.launches == 3 + 4 and loop.syncs == n // K and a.target_steps == target_counter(a) == n
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert_same(a, ref, opt)
    assert torch.equal(loss, ref_loss)
    assert not torch.equal(a.target_net.flat, torch.from_numpy(synth.brain_flat(synth.brain_state_dict(1))).to(dev))
    assert not torch.equal(a.target_net.flat, a.policy_net.flat)               # 28 is not a multiple of 5: three steps after the last sync


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_soft_graphed_loop_equals_coin_steps_with_a_cpu_lerp(dev, replay, opt):
    """tau = 0.01, GraphedDqnLoop with block 8 over 24 steps against the coin agent whose target is pulled to the host, lerp_-ed by CPU torch
    and pushed back after every step; every full block is one launch and no random number is drawn."""
    from ivos_w_amd.models.agent import GraphedDqnLoop
    B, seed, n, tau = 64, 78, 24, 0.01

    def lerp(a, k):
        t = a.target_net.flat.cpu()
        t.lerp_(a.policy_net.flat.cpu(), tau)
        a.target_net.flat.copy_(t)
    ref, ref_loss = coin_reference(dev, replay, B, seed, n, OPTS[opt], lerp)
    a = make_agent(dev, target_update="soft", tau=tau, **OPTS[opt])
    np.random.seed(11)
    before = np.random.get_state()
    loop = GraphedDqnLoop(a, replay, B, draw_seed=seed, block=8)
    loss = loop.run(n)
    after = np.random.get_state()
    assert loop.launches == n // 8 and loop.syncs == 0 and target_counter(a) == n
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert_same(a, ref, opt)
    assert torch.equal(loss, ref_loss)
    start = torch.from_numpy(synth.brain_flat(synth.brain_state_dict(1))).to(dev)
    assert int((a.target_net.flat != start).sum()) > 100000


# ------------------------------------------------------------------------------------------------------------------- the loops agree
def _run_loop(dev, replay, kind, n, B, seed, **opt):
    from ivos_w_amd.models.agent import AutoDqnLoop, CapturedDqnStep, GraphedDqnLoop, LeanDqnLoop
    from ivos_w_amd.models.momory_pool import draw_indices
    a = make_agent(dev, **opt)
    np.random.seed(5)
    loss = None
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "eager":
            for k in range(n):
                a.update_agent(replay.sample(torch.from_numpy(draw_indices(seed, k, B, len(replay))).to(dev)))
            loss = torch.tensor([a.loss[(a.loss_position - 1) % a.loss_capacity]], dtype=torch.float32)
        elif kind == "captured":                       # rows written by the caller: the chain gather -> loss -> update -> rule
            step = CapturedDqnStep(a, replay, B, fused=True)
            for k in range(n):
                step.idx.copy_(torch.from_numpy(draw_indices(seed, k, B, len(replay))).to(dev))
                loss = step.launch()
                if not step.tgt:
                    a.target_step()
        elif kind == "grads_only":                     # the data-parallel step's graph: the caller updates and applies the rule
            step = CapturedDqnStep(a, replay, B, fused=False)
            for k in range(n):
                step.idx.copy_(torch.from_numpy(draw_indices(seed, k, B, len(replay))).to(dev))
                loss = step.launch()
                a.apply_gradients()
                a.target_step()
        elif kind == "graphed":
            loop = GraphedDqnLoop(a, replay, B, draw_seed=seed, block=8)
            loss = loop.run(n - 3)
            loss = loop.run(3)
        elif kind == "lean":
            loss = LeanDqnLoop(a, replay, B, draw_seed=seed).run(n)
        else:
            loss = AutoDqnLoop(a, replay, B, draw_seed=seed, block=8, probe=8).run(n)
    return a, loss.cpu().clone()


@pytest.mark.parametrize("mode", ["soft", "periodic"])
@pytest.mark.parametrize("opt", ["adam", "sgd_poly"])
def test_every_loop_gives_the_same_result(dev, replay, mode, opt):
    """21 steps through update_agent, the captured chains (rows from the caller; gradients only), GraphedDqnLoop, LeanDqnLoop and AutoDqnLoop:
    the same parameters, target, optimizer state, counters and last loss."""
    rule = dict(target_update="soft", tau=0.05) if mode == "soft" else dict(target_update="periodic", target_period=4)
    n, B, seed = 21, 64, 99
    ref, ref_loss = _run_loop(dev, replay, "eager", n, B, seed, **rule, **OPTS[opt])
    assert ref.target_steps == target_counter(ref) == n
    for kind in ("captured", "grads_only", "graphed", "lean", "auto"):
        a, loss = _run_loop(dev, replay, kind, n, B, seed, **rule, **OPTS[opt])
        assert a.target_steps == target_counter(a) == n, kind
        assert torch.equal(a.policy_net.flat, ref.policy_net.flat), kind
        assert torch.equal(a.target_net.flat, ref.target_net.flat), kind
        for key in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            if ref.optimizer.state.get(key) is not None:
                assert torch.equal(a.optimizer.state[key], ref.optimizer.state[key]), (kind, key)
        assert torch.equal(loss, ref_loss), kind


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_period_one_equals_the_coin_that_always_fires(dev, replay, opt):
    n, B, seed = 10, 64, 31
    coin, coin_loss = _run_loop(dev, replay, "graphed", n, B, seed, update_rate=1.0, **OPTS[opt])
    one, one_loss = _run_loop(dev, replay, "graphed", n, B, seed, update_rate=0.0, target_update="periodic", target_period=1, **OPTS[opt])
    assert_same(coin, one, opt)
    assert torch.equal(coin_loss, one_loss) and torch.equal(one.target_net.flat, one.policy_net.flat)


@pytest.mark.parametrize("mode", ["coin", "soft", "periodic"])
def test_device_update_loop_equals_the_per_batch_loop(dev, monkeypatch, mode):
    """utils_agent._device_update_loop (train_agent.py's path) against update_agent per collated batch, two episodes of 10 steps."""
    from torch.utils.data import DataLoader
    from ivos_w_amd.datasets.agent_dataset import DAVIS2017AgentTrain
    from ivos_w_amd.utils import utils_agent
    rule = dict(coin=dict(update_rate=0.3), soft=dict(target_update="soft", tau=0.02), periodic=dict(target_update="periodic", target_period=3))[mode]
    ds = DAVIS2017AgentTrain.from_soa(synth.replay_transitions(n=300, T=25, seed=3))
    out, printed = {}, {}
    for path in ("host", "device"):
        monkeypatch.setenv("IVOSW_UPDATE_PATH", "host" if path == "host" else "")
        torch.manual_seed(123)
        np.random.seed(5)
        agent = make_agent(dev, **rule)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            for episode in range(2):
                loader = DataLoader(ds, batch_size=32, shuffle=True, num_workers=0)
                got = utils_agent._device_update_loop(agent, loader, 14)
                if path == "host":
                    assert got is None
                    for i, sample in enumerate(loader):
                        if i == 14:
                            break
                        agent.update_agent(sample)
        out[path], printed[path] = agent, buf.getvalue().count("target_net updated!")
    assert out["host"].optimizer.state["step"] == out["device"].optimizer.state["step"] == 20
    assert_same(out["host"], out["device"], mode)
    assert printed["host"] == printed["device"]
    if mode == "periodic":
        assert printed["device"] == 20 // 3
    if mode != "coin":
        assert target_counter(out["device"]) == out["device"].target_steps == 20


def test_prioritized_chain_composes(dev):
    """agent.replay = "prioritized" with the periodic rule: the captured 8-step graph and the lean loop against the eager chain with an
    explicit sync_target() every K-th step."""
    from ivos_w_amd.models.agent import GraphedDqnLoop, LeanDqnLoop
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    tr = synth.replay_transitions(n=3000, T=25, seed=5)
    B, seed, n, K = 64, 77, 16, 3
    res = {}
    for mode in ("eager", "graphed", "lean"):
        rule = dict() if mode == "eager" else dict(target_update="periodic", target_period=K)
        a = make_agent(dev, update_rate=0.0, replay="prioritized", **rule)
        rp = PrioritizedReplay(tr, dev, a.per_alpha, a.per_beta, a.per_beta_steps, a.per_eps, seed=seed)
        if mode == "eager":
            out = rp.new_batch(B)
            for k in range(1, n + 1):
                rp.sample_prioritized(B, out=out)
                a.loss_and_grads(out)
                a.optimizer.step()
                rp.update_priorities(out["idx"], out["td"])
                if k % K == 0:
                    a.sync_target()
        elif mode == "graphed":
            loop = GraphedDqnLoop(a, rp, B, draw_seed=seed, block=8)
            loop.run(n)
            assert loop.launches == 2 and loop.syncs == n // K
        else:
            lp = LeanDqnLoop(a, rp, B, draw_seed=seed)
            lp.run(n)
            assert lp.syncs == n // K
        res[mode] = (a.policy_net.flat.clone(), a.target_net.flat.clone(), rp.tree.clone(), rp.state.clone())
    for mode in ("graphed", "lean"):
        for x, y in zip(res["eager"], res[mode]):
            assert torch.equal(x, y), mode


# ------------------------------------------------------------------------------------------------------------------- the graphs' shape
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_kernel_node_counts(dev, replay, opt):
    """A condition on the captured graphs: the uniform one-call chain has exactly 8 kernel nodes per step in every mode (the rule rides in
    the update's launch); every other chain has at most one node more than the same chain under "coin" (prioritized: at most 12)."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import PrioritizedReplay
    rules = dict(coin=dict(), soft=dict(target_update="soft", tau=0.01), periodic=dict(target_update="periodic", target_period=3))
    nodes = {}
    for mode, rule in rules.items():
        a = make_agent(dev, **rule, **OPTS[opt])
        nodes[mode, "onecall"] = CapturedDqnStep(a, replay, 64, fused=True, draw_seed=1).kernel_nodes
        nodes[mode, "onecall4"] = CapturedDqnStep(make_agent(dev, **rule, **OPTS[opt]), replay, 64, fused=True, draw_seed=1, steps=4).kernel_nodes
        nodes[mode, "rows"] = CapturedDqnStep(make_agent(dev, **rule, **OPTS[opt]), replay, 64, fused=True).kernel_nodes
        nodes[mode, "grads"] = CapturedDqnStep(make_agent(dev, **rule, **OPTS[opt]), replay, 64, fused=False).kernel_nodes
        p = make_agent(dev, replay="prioritized", **rule, **OPTS[opt])
        rp = PrioritizedReplay(synth.replay_transitions(n=3000, T=25, seed=5), dev, p.per_alpha, p.per_beta, p.per_beta_steps, p.per_eps, seed=9)
        nodes[mode, "per"] = CapturedDqnStep(p, rp, 64, fused=True, draw_seed=9).kernel_nodes
    print(opt, nodes)
    for mode in rules:
        assert nodes[mode, "onecall"] == 8 and nodes[mode, "onecall4"] == 32, (mode, nodes)
        assert nodes[mode, "grads"] == nodes["coin", "grads"], (mode, nodes)
        assert nodes["coin", "rows"] <= nodes[mode, "rows"] <= nodes["coin", "rows"] + 1, (mode, nodes)
        assert nodes["coin", "per"] <= nodes[mode, "per"] <= min(12, nodes["coin", "per"] + 1), (mode, nodes)


def test_changes_after_capture_are_refused(dev, replay):
    from ivos_w_amd.models.agent import CapturedDqnStep
    a = make_agent(dev, target_update="soft", tau=0.01)
    step = CapturedDqnStep(a, replay, 64, fused=True, draw_seed=3)
    step.launch()
    for change in (dict(tau=0.02), dict(target_update="periodic", target_period=4), dict(target_update="coin")):
        old = {k: getattr(a, k) for k in change}
        a.__dict__.update(change)
        with pytest.raises(RuntimeError, match="target_update, tau, target_period"):
            step.launch()
        a.__dict__.update(old)
    step.launch()
    b = make_agent(dev, target_update="periodic", target_period=4)
    step = CapturedDqnStep(b, replay, 64, fused=True, draw_seed=3)
    b.target_period = 5
    with pytest.raises(RuntimeError, match="target_period"):
        step.launch()
    b.target_period = 0
    with pytest.raises(ValueError, match="agent.target_period"):
        step.launch()
    c = make_agent(dev)                                  # a step captured under "coin" refuses a rule switched on later
    step = CapturedDqnStep(c, replay, 64, fused=True, draw_seed=3)
    c.target_update = "soft"
    c.tau = 0.01
    with pytest.raises(RuntimeError, match="target_update"):
        step.launch()
    assert a.target_steps == target_counter(a) == 2


@pytest.mark.parametrize("opt", ["adam", "sgd_poly"])
def test_resume(dev, replay, opt):
    """Periodic, K = 4: 6 steps, save (parameters, target, optimizer.state_dict(), Agent.target_state()), a fresh agent, load, 6 more = 12
    steps straight: the device counter resumes at 6, so the next syncs are steps 8 and 12."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    from ivos_w_amd.models.momory_pool import draw_indices
    B, K = 64, 4
    rule = dict(target_update="periodic", target_period=K, **OPTS[opt])
    idxs = [torch.from_numpy(draw_indices(3, s, B, len(replay))).to(dev) for s in range(12)]

    def run(agent, ks):
        step = CapturedDqnStep(agent, replay, B, fused=True)
        for k in ks:
            step.idx.copy_(idxs[k])
            step.launch()
    straight = make_agent(dev, **rule)
    run(straight, range(12))
    first = make_agent(dev, **rule)
    run(first, range(6))
    saved = dict(policy=first.policy_net.flat.clone(), target=first.target_net.flat.clone(), opt=first.optimizer.state_dict(),
                 tgt=first.target_state())
    assert saved["tgt"] == dict(target_update="periodic", target_steps=6)
    fresh = make_agent(dev, **rule)
    fresh.policy_net.flat.copy_(saved["policy"])
    fresh.target_net.flat.copy_(saved["target"])
    fresh.optimizer.load_state_dict(saved["opt"])
    fresh.load_target_state(saved["tgt"])
    run(fresh, range(6, 12))
    assert target_counter(fresh) == target_counter(straight) == 12
    assert_same(fresh, straight, "resume")
    lost = make_agent(dev, **rule)                       # without the counter the syncs land on other steps
    lost.policy_net.flat.copy_(saved["policy"])
    lost.target_net.flat.copy_(saved["target"])
    lost.optimizer.load_state_dict(saved["opt"])
    run(lost, range(6, 11))
    assert not torch.equal(lost.target_net.flat, saved["target"])             # its 4th step (step 10) synced
    mid = make_agent(dev, **rule)
    run(mid, range(11))
    assert not torch.equal(mid.target_net.flat, lost.target_net.flat)


# ------------------------------------------------------------------------------------------------------------------- data parallel
DP_STEPS, DP_B, DP_K = 5, 64, 2


def _batch(tr, idx):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.collate_np(tr, idx).items()}


def _collect(procs, q, n, timeout=600):
    """n results from the workers' queue.  Fails as soon as a worker reports an error or ends without a result, and never leaves a worker
    behind: whatever is still running at the end is killed."""
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


def _dp_worker(rank, world, port, q, collective, rule):
    from ivos_w_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      IVOSW_P2P="0" if collective == "backend" else "1")
    r, w, dev = parallel.init("gloo")
    assert dev.type == "cuda" and w == 2
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    agent = make_agent(dev, **rule)
    np.random.seed(5 + 1000 * rank)                       # the ranks' host generators differ: the rule must not look at them
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for s in range(DP_STEPS):
            idx = synth.minibatch_indices(s, n=2000, B=DP_B, seed=7)
            agent.update_agent(_batch(tr, idx[rank * (DP_B // 2):(rank + 1) * (DP_B // 2)]))
            out.append((agent.policy_net.flat.cpu().numpy().copy(), agent.target_net.flat.cpu().numpy().copy()))
    assert parallel.collective_path(agent.policy_net.flat_grad) == collective
    q.put((rank, out, float(np.random.random())))
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


@pytest.mark.parametrize("mode", ["soft", "periodic"])
@pytest.mark.parametrize("collective", ["backend", "p2p"])
def test_world2_replicas_stay_identical_without_a_shared_coin(collective, mode):
    """Two ranks on one device, half the batch each, differently seeded np.random: parameters and target bit-identical on both ranks after
    every one of 5 steps (K = 2: two syncs), and the target follows the rule applied to the rank's own parameters."""
    from ivos_w_amd.models.agent import target_update_mirror        # (without the feature: fail here, before any worker starts)
    rule = dict(target_update="soft", tau=0.05) if mode == "soft" else dict(target_update="periodic", target_period=DP_K)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_dp_worker, args=(r, 2, port, q, collective, rule)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (out, coin) for r, out, coin in _collect(procs, q, 2)}
    assert res[0][1] != res[1][1]                         # the host generators really differed
    for a, b in zip(res[0][0], res[1][0]):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    t = synth.brain_flat(synth.brain_state_dict(1)).astype(np.float32)
    for k, (p_k, t_k) in enumerate(res[0][0], 1):
        t = target_update_mirror(t, p_k, mode, tau=rule.get("tau"), period=rule.get("target_period"), k=k)
        np.testing.assert_array_equal(t_k.view(np.int32), t.view(np.int32), err_msg=f"step {k}")
    assert not np.array_equal(res[0][0][-1][1], synth.brain_flat(synth.brain_state_dict(1)))


# ------------------------------------------------------------------------------------------------------------------- train_agent.py
def test_train_agent_with_the_target_option(tmp_path):
    """train_agent.py with agent.target_update=periodic / soft completes on the synthetic session; the epoch log line names the mode,
    train_summary.json reports updates // period syncs under periodic, and the checkpoints of the three modes differ."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "train_agent.py")
    env = dict(os.environ, PYTHONPATH=root)
    res, hists = {}, {}
    for name, opt in (("periodic", ["agent.target_update=periodic", "agent.target_period=3"]), ("soft", ["agent.target_update=soft", "agent.tau=0.05"]),
                      ("coin", [])):
        d = tmp_path / name
        common = ["synthetic=1", "synth.n_sequences=2", "synth.n_frames=26", "synth.height=120", "synth.width=216", f"ckpt_dir={d}/weights",
                  f"report_save_dir={d}/results", f"agent.save_result_dir={d}/train", "num_epochs=2", "agent.train_batch_size=16", "agent.lr=1e-4"]
        r = subprocess.run([sys.executable, script, "with"] + opt + common, cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        hists[name] = json.load(open(d / "train" / "train_summary.json"))
        res[name] = torch.load(d / "weights" / "agent.pt")
        assert f" target: {name}" in r.stdout
        assert (" syncs: " in r.stdout) == (name == "periodic")
    for h in hists["periodic"]:
        assert h["target_update"] == "periodic" and h["updates"] > 0 and h["target_syncs"] == h["updates"] // 3, h
    assert all(h["target_update"] == "soft" and "target_syncs" not in h for h in hists["soft"])
    assert all(h["target_update"] == "coin" for h in hists["coin"])
    assert [h["updates"] for h in hists["periodic"]] == [h["updates"] for h in hists["coin"]]
    for other in ("soft", "coin"):
        assert any(not torch.equal(res["periodic"][k], res[other][k]) for k in res["periodic"]), other
