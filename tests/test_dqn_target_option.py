"""agent.target_update = "coin" | "soft" | "periodic" without a GPU: the CLI / YAML carry the option, Agent._target_option checks it, the
library exports the new entries and refuses bad arguments before it touches a pointer, and the host mirror of the device rule equals CPU
torch bit for bit (lerp_ under soft, copy_ every period-th step under periodic)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models.agent import Agent, target_update_mirror, target_update_option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AD(dict):
    __getattr__ = dict.__getitem__


def _target(c):
    return c.agent.target_update, c.agent.tau, c.agent.target_period


def test_cli_and_yaml_carry_the_option(tmp_path):
    assert _target(entry.parse_cli([])) == ("coin", 0.005, 20)
    assert _target(entry.parse_cli(["with", "agent.target_update=soft", "agent.tau=0.01"])) == ("soft", 0.01, 20)
    assert _target(entry.parse_cli(["with", "agent.target_update=periodic", "agent.target_period=7"])) == ("periodic", 0.005, 7)
    y = tmp_path / "c.yaml"
    y.write_text("agent:\n  target_update: periodic\n  target_period: 50\n  tau: 0.02\n")
    c = entry.parse_cli(["--config", str(y)])
    assert _target(c) == ("periodic", 0.02, 50)
    assert c.agent.update_rate == 0.05                                          # the rest of the section keeps its defaults
    assert Agent._target_option(c.agent) == ("periodic", None, 50)


def test_target_option_defaults_and_mode_local_checks():
    assert Agent._target_option(AD(update_rate=0.05)) == ("coin", None, None)   # a config without the keys keeps the coin
    assert Agent._target_option(AD(target_update="soft")) == ("soft", 0.005, None)
    assert Agent._target_option(AD(target_update="periodic")) == ("periodic", None, 20)
    assert Agent._target_option(AD(target_update="soft", tau=0.3, target_period=0)) == ("soft", 0.3, None)        # period not looked at
    assert Agent._target_option(AD(target_update="periodic", tau=7.0, target_period=3)) == ("periodic", None, 3)  # tau not looked at
    assert Agent._target_option(AD(target_update="coin", tau="x", target_period=-1)) == ("coin", None, None)
    assert Agent._target_option(AD(target_update="periodic", target_period=2 ** 31 - 1))[2] == 2 ** 31 - 1


BAD = [dict(target_update="Soft"), dict(target_update="PERIODIC"), dict(target_update="polyak"), dict(target_update=True),
       dict(target_update=None), dict(target_update=1),
       dict(target_update="soft", tau=True), dict(target_update="soft", tau="0.01"), dict(target_update="soft", tau=float("nan")),
       dict(target_update="soft", tau=float("inf")), dict(target_update="soft", tau=0), dict(target_update="soft", tau=0.0),
       dict(target_update="soft", tau=0.5), dict(target_update="soft", tau=1), dict(target_update="soft", tau=1.0),
       dict(target_update="soft", tau=-0.01), dict(target_update="soft", tau=None), dict(target_update="soft", tau=1e-60),
       dict(target_update="periodic", target_period=0), dict(target_update="periodic", target_period=-3),
       dict(target_update="periodic", target_period=2.5), dict(target_update="periodic", target_period=20.0),
       dict(target_update="periodic", target_period=2 ** 31), dict(target_update="periodic", target_period=True),
       dict(target_update="periodic", target_period="20"), dict(target_update="periodic", target_period=None)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v!r}" for k, v in b.items()))
def test_target_option_refuses(bad):
    with pytest.raises(ValueError, match="agent.target_update|agent.tau|agent.target_period"):
        Agent._target_option(AD(bad))


def test_soft_refusal_points_at_periodic():
    with pytest.raises(ValueError, match="periodic"):
        target_update_option("soft", 0.5, 20)


def test_new_entries_are_declared():
    S = L.SIGNATURES
    assert S["ivosw_target_state_bytes"] == (L._sz, [])
    assert S["ivosw_target_update"] == (L._i, [L._p, L._p, L._i, L._i, L._f, L._i, L._p, L._p])
    # the one-call step with the rule: the common head of the one-call entries, then the optimizer block, the rule, the stream
    ex, tg = S["ivosw_dqn_step_drawn_ex"][1], S["ivosw_dqn_step_drawn_tgt"][1]
    w = ex.index(L._sz)
    assert tg[:w + 1] == ex[:w + 1]
    assert tg[w + 1:] == [L._i, L._p, L._p, L._p, L._f, L._p, L._i] + [L._f] * 4 + [L._i] + [L._f] * 3 + [L._i, L._f, L._i, L._p] + [L._p]
    assert (L.TARGET_SOFT, L.TARGET_PERIODIC, L.OPT_ADAM, L.OPT_SGD) == (1, 2, 0, 1)
    hdr = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for name in ("ivosw_target_state_bytes", "ivosw_target_update", "ivosw_dqn_step_drawn_tgt", "IVOSW_TARGET_SOFT 1", "IVOSW_TARGET_PERIODIC 2",
                 "IVOSW_OPT_ADAM 0", "IVOSW_OPT_SGD 1"):
        assert name in hdr, name


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _fake():
    """A non-NULL pointer that must never be dereferenced: every case below is refused before any pointer is used."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def _msg(lib):
    return lib.ivosw_last_error().decode()


RULE_BAD = [(dict(state=None), "null target_state"), (dict(mode=0), "mode"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
            (dict(mode=1, tau=0.0), "tau"), (dict(mode=1, tau=0.5), "tau"), (dict(mode=1, tau=1.0), "tau"), (dict(mode=1, tau=-0.1), "tau"),
            (dict(mode=1, tau=float("nan")), "tau"), (dict(mode=1, tau=float("inf")), "tau"),
            (dict(mode=2, period=0), "period"), (dict(mode=2, period=-5), "period")]


def test_target_update_refuses_bad_arguments(lib):
    assert lib.ivosw_target_state_bytes() == 16
    name = "ivosw_target_update"
    for kw, word in RULE_BAD:                        # NULL data pointers: nothing can have been launched
        a = dict(state=_fake()[1], mode=1, tau=0.005, period=20)
        a.update(kw)
        assert lib.ivosw_target_update(None, None, 10, a["mode"], a["tau"], a["period"], a["state"], None) == -1, kw
        assert name in _msg(lib) and word in _msg(lib), (kw, _msg(lib))
    keep, p = _fake()
    keep2, q = _fake()
    assert lib.ivosw_target_update(None, q, 10, 1, 0.005, 20, p, None) == -1 and "null pointer" in _msg(lib)
    assert lib.ivosw_target_update(q, None, 10, 2, 0.0, 20, p, None) == -1 and "null pointer" in _msg(lib)
    assert lib.ivosw_target_update(q, q, 10, 2, 0.0, 20, p, None) == -1 and "different" in _msg(lib)
    assert lib.ivosw_target_update(q, p, 0, 2, 0.0, 20, p, None) == -1 and "n must be positive" in _msg(lib)
    # valid values reach the device-pointer check; the value of the other mode's parameter is not looked at
    assert lib.ivosw_target_update(q, p, 10, 1, 0.005, 0, p, None) == -1 and "not a device pointer" in _msg(lib)
    assert lib.ivosw_target_update(q, p, 10, 2, 9.0, 1, p, None) == -1 and "not a device pointer" in _msg(lib)


def _step_args(p, q, data=True, **over):
    a = dict(n=100, B=4, T=3, gamma=0.95, kind=L.DQN_LOSS_MSE, delta=1.0, opt=L.OPT_ADAM, buf0=p, buf1=p, ostate=p, lr=1e-3, table=None, steps=0,
             b1=0.9, b2=0.999, eps=1e-8, mu=0.0, nest=0, wd=0.0, mode=1, tau=0.005, period=20, state=p)
    a.update(over)
    d = p if data else None
    return [d, q if data else None] + [d] * 8 + [a["n"], a["B"], a["T"], a["gamma"], a["kind"], a["delta"]] + [d] * 9 + [1 << 20] + \
        [a["opt"], a["buf0"], a["buf1"], a["ostate"], a["lr"], a["table"], a["steps"], a["b1"], a["b2"], a["eps"], a["mu"], a["nest"], a["wd"],
         1.0, 1.0, a["mode"], a["tau"], a["period"], a["state"], None]


def test_one_call_target_step_refuses_bad_arguments(lib):
    keep, p = _fake()
    keep2, q = _fake()
    name = "ivosw_dqn_step_drawn_tgt"
    fn = lib.ivosw_dqn_step_drawn_tgt
    for kw, word in RULE_BAD:                        # with NULL data pointers: refused before anything else is looked at
        assert fn(*_step_args(p, q, data=False, **kw)) == -1, kw
        assert name in _msg(lib) and word in _msg(lib), (kw, _msg(lib))
    for i in (0, 1, 9, 22, 24):                      # policy, target, draw state, grads, ws
        args = _step_args(p, q)
        args[i] = None
        assert fn(*args) == -1 and "null pointer" in _msg(lib), i
    assert fn(*_step_args(p, p)) == -1 and "different" in _msg(lib)
    bad = [(dict(opt=2), "optimizer"), (dict(opt=-1), "optimizer"), (dict(buf0=None), "null"), (dict(buf1=None), "null"),
           (dict(ostate=None), "null"), (dict(opt=L.OPT_SGD, table=p, steps=8, ostate=None), "null"), (dict(n=0), "must be positive"),
           (dict(B=0), "must be positive"), (dict(T=-1), "must be positive"), (dict(kind=7), "loss kind"), (dict(table=p, steps=0), "lr_steps"),
           (dict(b1=1.5), "beta1"), (dict(b2=1.0), "beta2"), (dict(eps=-1.0), "eps"), (dict(wd=float("inf")), "weight_decay"),
           (dict(opt=L.OPT_SGD, mu=-0.5), "momentum"), (dict(opt=L.OPT_SGD, nest=2), "nesterov"), (dict(opt=L.OPT_SGD, mu=0.0, nest=1), "nesterov"),
           (dict(opt=L.OPT_SGD, lr=float("nan")), "lr"), (dict(opt=L.OPT_SGD, wd=-1.0), "weight_decay")]
    for over, word in bad:
        assert fn(*_step_args(p, q, **over)) == -1, over
        assert name in _msg(lib) and word in _msg(lib), (over, _msg(lib))
    # valid values of every optimizer / schedule combination reach the device-pointer check
    for over in (dict(), dict(table=p, steps=8), dict(opt=L.OPT_SGD, mu=0.9, buf1=None, ostate=None),
                 dict(opt=L.OPT_SGD, mu=0.9, nest=1, table=p, steps=8, buf1=None), dict(mode=2, tau=0.0, period=1)):
        assert fn(*_step_args(p, q, **over)) == -1 and "not a device pointer" in _msg(lib), (over, _msg(lib))


def test_version_is_unchanged(lib):
    assert lib.ivosw_version() == 102


def test_target_kernels_do_not_spill_and_the_old_tails_are_still_there(lib):
    """The new kernels in the shipped library: no spill, no scratch; the fused tails need no more registers than the tails they extend."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    table = kr.kernel_table(L.LIB_PATH)
    pick = lambda key: [r for n, r in table.items() if key in n]
    for key, count in (("target_update_kernel", 2), ("adam_tail_tgt_kernel", 2), ("sgd_tail_tgt_kernel", 2)):
        hits = pick(key)
        assert len(hits) == count, (key, hits)
        assert all(r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 for r in hits), (key, hits)
    for new, old in (("adam_tail_tgt_kernel", "clamp_adam_dev_reduce_kernel"), ("sgd_tail_tgt_kernel", "clamp_sgd_reduce_sched_kernel")):
        (o,) = pick(old)
        assert all(r["vgpr"] <= o["vgpr"] for r in pick(new)), (new, pick(new), o)


@pytest.mark.parametrize("tau", [0.005, 0.01, 0.05, 0.3, 0.499])
def test_soft_mirror_equals_torch_lerp(tau):
    """target_update_mirror("soft") == torch.Tensor.lerp_(p, tau) on the CPU, bit for bit, over 24 applications with policies of mixed
    magnitude (cancellation, tiny and large steps)."""
    rng = np.random.RandomState(int(tau * 1000))
    n = L.BRAIN_NPARAMS
    t = rng.randn(n).astype(np.float32)
    tt = torch.from_numpy(t.copy())
    for k in range(1, 25):
        p = (rng.randn(n) * 10.0 ** rng.uniform(-4, 2)).astype(np.float32)
        if k % 5 == 0:
            p[::3] = t[::3]                                                   # exact fixed points
        t = target_update_mirror(t, p, "soft", tau=tau, k=k)
        tt.lerp_(torch.from_numpy(p), tau)
        assert t.dtype == np.float32
        np.testing.assert_array_equal(t.view(np.int32), tt.numpy().view(np.int32), err_msg=f"step {k}")


@pytest.mark.parametrize("period", [1, 3, 20])
def test_periodic_mirror_equals_torch_copy(period):
    rng = np.random.RandomState(period)
    t = rng.randn(1001).astype(np.float32)
    tt = torch.from_numpy(t.copy())
    for k in range(1, 45):
        p = rng.randn(1001).astype(np.float32)
        t = target_update_mirror(t, p, "periodic", period=period, k=k)
        if k % period == 0:
            tt.copy_(torch.from_numpy(p))
        np.testing.assert_array_equal(t.view(np.int32), tt.numpy().view(np.int32), err_msg=f"step {k}")
    with pytest.raises(ValueError):
        target_update_mirror(t, t, "coin")


def test_coin_mode_draws_the_reference_coin_and_the_others_draw_nothing(monkeypatch):
    """Agent.target_step without a GPU (the launches replaced): coin = one np.random draw per step, a sync when it is below update_rate, as
    Agent.update_agent always did; soft / periodic draw nothing and report steps // period hard syncs."""
    calls = []
    a = object.__new__(Agent)
    a.__dict__.update(target_update="coin", tau=None, target_period=None, update_rate=0.3, target_steps=0, _target_dev=None, _target_dev_step=0)
    monkeypatch.setattr(Agent, "sync_target", lambda self: calls.append("sync"))
    monkeypatch.setattr(Agent, "target_dev_state", lambda self: None)
    monkeypatch.setattr(Agent, "enqueue_target_update", lambda self: calls.append("rule"))
    np.random.seed(5)
    fired = [a.target_step() for _ in range(50)]
    np.random.seed(5)
    want = [bool(np.random.random() < 0.3) for _ in range(50)]
    assert fired == want and calls == ["sync"] * sum(want) and a.target_steps == 0
    for mode, kw, n_sync in (("soft", dict(tau=0.01), 0), ("periodic", dict(target_period=7), 50 // 7)):
        del calls[:]
        a.__dict__.update(target_update=mode, tau=None, target_period=None, target_steps=0)
        a.__dict__.update(kw)
        state = np.random.get_state()
        fired = [a.target_step() for _ in range(50)]
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert calls == ["rule"] * 50 and sum(fired) == n_sync and a.target_steps == 50
        if mode == "periodic":
            assert [i + 1 for i, f in enumerate(fired) if f] == list(range(7, 51, 7))
    assert a.target_state() == dict(target_update="periodic", target_steps=50)
    a.load_target_state(dict(target_update="periodic", target_steps=13))
    assert a.target_steps == 13
    with pytest.raises(ValueError, match="soft"):
        a.load_target_state(dict(target_update="soft", target_steps=1))
