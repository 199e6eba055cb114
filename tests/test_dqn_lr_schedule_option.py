"""The learning-rate schedule option (cfg.agent.lr_schedule = "constant" | "poly", cfg.agent.lr_pow, cfg.agent.lr_total_steps) on the host
side, no GPU: the CLI and YAML carry it to the agent block with the reference's defaults, the agent refuses what it cannot run, the host
table is torch's PolynomialLR closed form bit for bit, the C binding declares the four scheduled entries in line with their constant-lr
counterparts, the built library refuses bad arguments before it touches a pointer, and the new kernels neither spill nor use scratch."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AD(dict):
    __getattr__ = dict.__getitem__


def test_cli_carries_the_schedule_option():
    c = entry.parse_cli(["with", "agent.lr_schedule=poly", "agent.lr_total_steps=2000", "agent.lr_pow=0.5"])
    assert (c.agent.lr_schedule, c.agent.lr_pow, c.agent.lr_total_steps) == ("poly", 0.5, 2000)
    assert isinstance(c.agent.lr_total_steps, int)


def test_defaults_are_the_references_constant_lr():
    c = entry.parse_cli([])
    assert (c.agent.lr_schedule, c.agent.lr_pow, c.agent.lr_total_steps) == ("constant", 0.9, 0)
    assert (c.agent.optimizer, c.agent.lr, c.agent.momentum, c.agent.loss, c.agent.gamma) == ("adam", 5e-6, 0.9, "mse", 0.95)


def test_yaml_config_carries_the_schedule_option(tmp_path):
    p = tmp_path / "cfg.yaml"
    p.write_text("agent:\n  lr_schedule: poly\n  lr_total_steps: 2000\n  lr_pow: 0.9\n")
    c = entry.parse_cli(["--config", str(p)])
    assert (c.agent.lr_schedule, c.agent.lr_pow, c.agent.lr_total_steps) == ("poly", 0.9, 2000)
    assert c.agent.gamma == 0.95 and c.agent.optimizer == "adam" and c.agent.lr == 5e-6      # the rest keeps its defaults


def test_agent_reads_the_option_and_refuses_the_unknown():
    from ivos_w_amd.models.agent import LR_TOTAL_STEPS_MAX, Agent
    opt = Agent._lr_schedule_option
    assert opt(AD(gamma=0.95)) == ("constant", None, None)                 # configs without the keys keep the constant lr
    assert opt(AD(lr_schedule="constant", lr_pow="junk", lr_total_steps=-3)) == ("constant", None, None)   # only checked under poly
    assert opt(AD(entry.parse_cli([]).agent)) == ("constant", None, None)  # the reference's own block
    assert opt(AD(lr_schedule="poly", lr_total_steps=2000)) == ("poly", 0.9, 2000)
    assert opt(AD(lr_schedule="poly", lr_total_steps=1, lr_pow=1)) == ("poly", 1.0, 1)
    assert opt(AD(lr_schedule="poly", lr_total_steps=LR_TOTAL_STEPS_MAX, lr_pow=0.0)) == ("poly", 0.0, LR_TOTAL_STEPS_MAX)
    assert LR_TOTAL_STEPS_MAX == 1 << 24
    for bad in (dict(lr_schedule="Poly"), dict(lr_schedule="POLY"), dict(lr_schedule="cosine"), dict(lr_schedule=None),
                dict(lr_schedule="Constant"), dict(lr_schedule="poly"), dict(lr_schedule="poly", lr_total_steps=0),
                dict(lr_schedule="poly", lr_total_steps=-5), dict(lr_schedule="poly", lr_total_steps=2000.0),
                dict(lr_schedule="poly", lr_total_steps="2000"), dict(lr_schedule="poly", lr_total_steps=True),
                dict(lr_schedule="poly", lr_total_steps=LR_TOTAL_STEPS_MAX + 1),
                dict(lr_schedule="poly", lr_total_steps=10, lr_pow=float("nan")), dict(lr_schedule="poly", lr_total_steps=10, lr_pow=float("inf")),
                dict(lr_schedule="poly", lr_total_steps=10, lr_pow=-0.5), dict(lr_schedule="poly", lr_total_steps=10, lr_pow=True),
                dict(lr_schedule="poly", lr_total_steps=10, lr_pow="0.9"), dict(lr_schedule="poly", lr_total_steps=10, lr_pow=None)):
        with pytest.raises(ValueError):
            opt(AD(bad))


def _closed_form(lr, lr_pow, n, k):
    """torch.optim.lr_scheduler.PolynomialLR._get_closed_form_lr at last_epoch = k, rounded to float32."""
    return np.float32(lr * (1.0 - min(n, k) / n) ** lr_pow)


@pytest.mark.parametrize("lr,lr_pow,n", [(5e-6, 0.9, 2000), (1e-3, 0.9, 8), (1e-3, 1.0, 8), (1e-3, 0.0, 8), (3e-4, 0.9, 1),
                                         (0.1, 2.5, 37), (1e-3, 0.9, 100003)])
def test_host_table_is_the_closed_form_bit_for_bit(lr, lr_pow, n):
    from ivos_w_amd.models.agent import poly_lr_table
    t = poly_lr_table(lr, lr_pow, n)
    assert t.dtype == np.float32 and t.shape == (n + 1,)
    want = np.array([_closed_form(lr, lr_pow, n, k) for k in range(n + 1)], dtype=np.float32)
    np.testing.assert_array_equal(t.view(np.uint32), want.view(np.uint32))
    assert t[0] == np.float32(lr)
    assert t[n] == (np.float32(lr) if lr_pow == 0.0 else 0.0)               # Python: 0.0 ** 0 == 1.0


def test_optimizer_lr_follows_the_table_past_n():
    """lr_at(k) / current_lr() on both optimizers (host only: no kernel is launched): the table's entry min(k, N), 0 from k = N on."""
    import torch
    from ivos_w_amd.models.agent import Brain, FusedClampAdam, FusedClampSGD
    brain = Brain()
    for make in (lambda **s: FusedClampAdam(brain, lr=1e-3, weight_decay=0.0, **s),
                 lambda **s: FusedClampSGD(brain, lr=1e-3, weight_decay=0.0, momentum=0.9, **s)):
        opt = make(lr_schedule="poly", lr_pow=0.9, lr_total_steps=8)
        assert opt.scheduled and opt.schedule() == ("poly", 1e-3, 0.9, 8)
        for k in range(14):
            assert opt.lr_at(k) == float(_closed_form(1e-3, 0.9, 8, k)), k
        assert opt.lr_at(8) == opt.lr_at(13) == 0.0
        opt.state["step"] = 5
        assert opt.current_lr() == float(_closed_form(1e-3, 0.9, 8, 5))
        pg = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
        assert (pg["lr_schedule"], pg["lr_pow"], pg["lr_total_steps"]) == ("poly", 0.9, 8)
        const = make()
        assert not const.scheduled and const.current_lr() == 1e-3 and const.lr_at(10 ** 6) == 1e-3
        assert const._schedule_hyper() == ("constant", None, None, 0)
        # a state dict carries the schedule in its param_groups; loading it restores the schedule
        const._load_schedule(dict(param_groups=[pg]))
        assert const.schedule() == ("poly", 1e-3, 0.9, 8)
        with pytest.raises(ValueError):
            const._load_schedule(dict(param_groups=[dict(pg, lr_schedule="cosine")]))
        with pytest.raises(ValueError):
            make(lr_schedule="poly", lr_pow=0.9, lr_total_steps=0)
    assert torch.is_tensor(brain.flat)


def test_the_scheduled_entries_are_bound_in_line_with_the_constant_ones():
    S = L.SIGNATURES
    for name in ("ivosw_clamp_adam_dev_sched", "ivosw_clamp_sgd_dev_sched", "ivosw_dqn_step_drawn_sched", "ivosw_dqn_step_drawn_sgd_sched"):
        assert name in S and S[name][0] is L._i, name
    assert S["ivosw_sgd_state_bytes"] == (L._sz, [])
    # clamp_adam_dev_sched: clamp_adam_dev with (lr_table, lr_steps) in place of lr
    adam = S["ivosw_clamp_adam_dev"][1]
    assert S["ivosw_clamp_adam_dev_sched"][1] == adam[:6] + [L._p, L._i] + adam[7:]
    # clamp_sgd_dev_sched: clamp_sgd with sgd_state after n and (lr_table, lr_steps) in place of lr
    sgd = S["ivosw_clamp_sgd"][1]
    assert S["ivosw_clamp_sgd_dev_sched"][1] == sgd[:4] + [L._p, L._p, L._i] + sgd[5:]
    # the one-call steps: the constant-lr entry with the same substitutions
    ex, sch = S["ivosw_dqn_step_drawn_ex"][1], S["ivosw_dqn_step_drawn_sched"][1]
    w = ex.index(L._sz)
    assert sch == ex[:w + 4] + [L._p, L._i] + ex[w + 5:]
    sg, sgs = S["ivosw_dqn_step_drawn_sgd"][1], S["ivosw_dqn_step_drawn_sgd_sched"][1]
    assert sgs == sg[:w + 2] + [L._p, L._p, L._i] + sg[w + 3:]


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


def test_clamp_adam_dev_sched_refuses_bad_arguments(lib):
    keep, p = _fake()
    name = "ivosw_clamp_adam_dev_sched"

    def call(params=p, state=p, table=p, steps=8, n=10, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        return lib.ivosw_clamp_adam_dev_sched(params, p, p, p, n, state, table, steps, b1, b2, eps, wd, 1.0, 1.0, None)
    for kw, word in ((dict(params=None), "null"), (dict(state=None), "null"), (dict(n=0), "n must be positive"), (dict(table=None), "lr_table"),
                     (dict(steps=0), "lr_steps"), (dict(steps=-1), "lr_steps"), (dict(b1=1.0), "beta1"), (dict(b1=float("nan")), "beta1"),
                     (dict(b2=-0.1), "beta2"), (dict(eps=-1e-8), "eps"), (dict(eps=float("inf")), "eps"), (dict(wd=-5e-4), "weight_decay")):
        assert call(**kw) == -1, kw
        assert name in _msg(lib) and word in _msg(lib), (kw, _msg(lib))
    assert call() == -1 and "not a device pointer" in _msg(lib)           # valid values reach the device-pointer check


SGD_BAD = [(dict(mu=-0.5), "momentum"), (dict(mu=float("nan")), "momentum"), (dict(wd=-5e-4), "weight_decay"),
           (dict(wd=float("nan")), "weight_decay"), (dict(nest=2), "nesterov"), (dict(mu=0.0, nest=1), "nesterov")]


def test_clamp_sgd_dev_sched_refuses_bad_arguments(lib):
    keep, p = _fake()
    name = "ivosw_clamp_sgd_dev_sched"

    def call(params=p, buf=p, state=p, table=p, steps=8, n=10, mu=0.9, wd=0.0, nest=0):
        return lib.ivosw_clamp_sgd_dev_sched(params, p, buf, n, state, table, steps, mu, wd, nest, 1.0, 1.0, None)
    for kw, word in [(dict(params=None), "null"), (dict(buf=None), "null"), (dict(state=None), "null"), (dict(n=0), "n must be positive"),
                     (dict(table=None), "lr_table"), (dict(steps=0), "lr_steps")] + SGD_BAD:
        assert call(**kw) == -1, kw
        assert name in _msg(lib) and word in _msg(lib), (kw, _msg(lib))
    assert call() == -1 and "not a device pointer" in _msg(lib)
    assert lib.ivosw_sgd_state_bytes() == 8


def _step_args(p, sgd, **over):
    a = dict(n=100, B=4, T=3, gamma=0.95, kind=L.DQN_LOSS_MSE, delta=1.0, table=p, steps=8, b1=0.9, b2=0.999, eps=1e-8, mu=0.9, wd=0.0, nest=0)
    a.update(over)
    head = [p] * 10 + [a["n"], a["B"], a["T"], a["gamma"], a["kind"], a["delta"]] + [p] * 9 + [1 << 20]
    if sgd:
        return head + [p, p, a["table"], a["steps"], a["mu"], a["wd"], a["nest"], 1.0, 1.0, None]
    return head + [p, p, p, a["table"], a["steps"], a["b1"], a["b2"], a["eps"], a["wd"], 1.0, 1.0, None]


@pytest.mark.parametrize("sgd", [False, True])
def test_one_call_sched_steps_refuse_bad_arguments(lib, sgd):
    keep, p = _fake()
    name = "ivosw_dqn_step_drawn_sgd_sched" if sgd else "ivosw_dqn_step_drawn_sched"
    fn = getattr(lib, name)
    for i in (0, 26, 27, 28 if not sgd else 27):                         # policy, the optimizer's buffers / state
        args = _step_args(p, sgd)
        args[i] = None
        assert fn(*args) == -1 and "null" in _msg(lib), i
    for over in (dict(n=0), dict(B=0), dict(T=-1)):
        assert fn(*_step_args(p, sgd, **over)) == -1 and "must be positive" in _msg(lib), over
    assert fn(*_step_args(p, sgd, kind=7)) == -1 and "loss kind" in _msg(lib)
    bad = [(dict(table=None), "lr_table"), (dict(steps=0), "lr_steps"), (dict(steps=-2), "lr_steps")]
    bad += SGD_BAD if sgd else [(dict(b1=1.5), "beta1"), (dict(b2=1.0), "beta2"), (dict(eps=-1.0), "eps"), (dict(wd=float("inf")), "weight_decay")]
    for over, word in bad:
        assert fn(*_step_args(p, sgd, **over)) == -1, over
        assert name in _msg(lib) and word in _msg(lib), (over, _msg(lib))
    assert fn(*_step_args(p, sgd)) == -1 and "not a device pointer" in _msg(lib)


def test_version_is_unchanged(lib):
    assert lib.ivosw_version() == 102


def test_scheduled_kernels_do_not_spill(lib):
    """The new kernels in the shipped library: no spill, no scratch, register counts within the budget test_cabi.py applies."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    table = kr.kernel_table(L.LIB_PATH)
    for key, count in (("clamp_adam_dev_sched_kernel", 2), ("clamp_sgd_sched_kernel", 2), ("clamp_adam_dev_reduce_sched_kernel", 1),
                       ("clamp_sgd_reduce_sched_kernel", 1)):
        hits = [r for n, r in table.items() if key in n]
        assert len(hits) == count, (key, hits)
        assert all(r["spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 512 and r["lds"] <= 163840 for r in hits), (key, hits)
