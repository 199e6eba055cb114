"""The optimizer option (cfg.agent.optimizer = "adam" | "sgd", cfg.agent.momentum, cfg.agent.nesterov) on the host side, no GPU: the CLI and
YAML carry it to the agent block, the defaults keep the reference's Adam, the agent refuses what it cannot run, the C binding declares the
three SGD entries in line with their Adam counterparts, and the built library refuses bad hyper-parameters before it touches a pointer."""
import ctypes

import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry


class AD(dict):
    __getattr__ = dict.__getitem__


def test_cli_carries_the_optimizer_option():
    c = entry.parse_cli(["with", "agent.optimizer=sgd", "agent.momentum=0.5", "agent.nesterov=true"])
    assert (c.agent.optimizer, c.agent.momentum, c.agent.nesterov) == ("sgd", 0.5, True)


def test_defaults_are_the_references_adam():
    c = entry.parse_cli([])
    assert (c.agent.optimizer, c.agent.momentum, c.agent.nesterov) == ("adam", 0.9, False)
    assert c.agent.nesterov is False


def test_yaml_config_carries_the_optimizer_option(tmp_path):
    p = tmp_path / "cfg.yaml"
    p.write_text("agent:\n  optimizer: sgd\n  momentum: 0.5\n  nesterov: true\n")
    c = entry.parse_cli(["--config", str(p)])
    assert (c.agent.optimizer, c.agent.momentum, c.agent.nesterov) == ("sgd", 0.5, True)
    assert c.agent.gamma == 0.95 and c.agent.loss == "mse"         # the rest of the block keeps its defaults


def test_agent_reads_the_option_and_refuses_the_unknown():
    from ivos_w_amd.models.agent import Agent
    assert Agent._optimizer_option(AD(gamma=0.95)) == ("adam", 0.0, False)      # configs without the keys (bench.py, older tests) stay Adam
    assert Agent._optimizer_option(AD(optimizer="sgd")) == ("sgd", 0.0, False)
    assert Agent._optimizer_option(AD(optimizer="sgd", momentum=0.9, nesterov=True)) == ("sgd", 0.9, True)
    assert Agent._optimizer_option(AD(optimizer="sgd", momentum=1)) == ("sgd", 1.0, False)
    assert Agent._optimizer_option(AD(optimizer="adam", momentum=0.9)) == ("adam", 0.9, False)
    for bad in (dict(optimizer="rmsprop"), dict(optimizer="SGD"), dict(optimizer="Adam"), dict(optimizer="adamw"), dict(optimizer=None),
                dict(optimizer="sgd", momentum=-0.1), dict(optimizer="sgd", momentum=float("nan")), dict(optimizer="sgd", momentum=float("inf")),
                dict(optimizer="sgd", momentum="0.9"), dict(optimizer="sgd", momentum=True), dict(optimizer="sgd", momentum=0.9, nesterov=1),
                dict(optimizer="sgd", momentum=0.9, nesterov="true"), dict(optimizer="sgd", nesterov=True),
                dict(optimizer="sgd", momentum=0.0, nesterov=True)):
        with pytest.raises(ValueError):
            Agent._optimizer_option(AD(bad))


def test_the_sgd_entries_are_bound_in_line_with_adam():
    S = L.SIGNATURES
    for name in ("ivosw_clamp_sgd", "ivosw_dqn_step_drawn_sgd", "ivosw_p2p_allreduce_clamp_sgd"):
        assert name in S and S[name][0] is L._i, name
    # clamp_sgd: (params, grads, momentum_buf, n, lr, momentum, weight_decay, nesterov, clamp, grad_scale, stream)
    assert S["ivosw_clamp_sgd"][1] == [L._p, L._p, L._p, L._i, L._f, L._f, L._f, L._i, L._f, L._f, L._p]
    # the one-call step: ivosw_dqn_step_drawn_ex's arguments up to ws_bytes, then the SGD tail
    ex, sgd = S["ivosw_dqn_step_drawn_ex"][1], S["ivosw_dqn_step_drawn_sgd"][1]
    w = ex.index(L._sz)
    assert sgd[:w + 1] == ex[:w + 1]
    assert sgd[w + 1:] == [L._p, L._f, L._f, L._f, L._i, L._f, L._f, L._p]
    # P2P: ivosw_p2p_allreduce_clamp_adam's arguments up to params, then momentum_buf and the SGD hyper-parameters
    adam, psgd = S["ivosw_p2p_allreduce_clamp_adam"][1], S["ivosw_p2p_allreduce_clamp_sgd"][1]
    assert psgd[:9] == adam[:9]
    assert psgd[9:] == [L._p, L._f, L._f, L._f, L._i, L._f, L._p]


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


# (lr, momentum, weight_decay, nesterov) -> the word the error message must carry
BAD = [((-1e-3, 0.9, 0.0, 0), "lr"), ((float("nan"), 0.9, 0.0, 0), "lr"), ((float("inf"), 0.9, 0.0, 0), "lr"),
       ((1e-3, -0.5, 0.0, 0), "momentum"), ((1e-3, float("nan"), 0.0, 0), "momentum"), ((1e-3, float("inf"), 0.0, 0), "momentum"),
       ((1e-3, 0.9, -5e-4, 0), "weight_decay"), ((1e-3, 0.9, float("nan"), 0), "weight_decay"),
       ((1e-3, 0.9, 0.0, 2), "nesterov"), ((1e-3, 0.9, 0.0, -1), "nesterov"), ((1e-3, 0.0, 0.0, 1), "nesterov")]


def _fake():
    """A non-NULL pointer that must never be dereferenced: every case below is refused before any pointer is used."""
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_clamp_sgd_refuses_bad_arguments(lib):
    keep, p = _fake()
    assert lib.ivosw_clamp_sgd(None, p, p, 10, 1e-3, 0.9, 0.0, 0, 1.0, 1.0, None) == -1
    assert b"null" in lib.ivosw_last_error()
    assert lib.ivosw_clamp_sgd(p, p, p, 0, 1e-3, 0.9, 0.0, 0, 1.0, 1.0, None) == -1
    assert b"n must be positive" in lib.ivosw_last_error()
    for (lr, mu, wd, nest), word in BAD:
        assert lib.ivosw_clamp_sgd(p, p, p, 10, lr, mu, wd, nest, 1.0, 1.0, None) == -1, (lr, mu, wd, nest)
        msg = lib.ivosw_last_error().decode()
        assert f"{word} must" in msg or (word == "nesterov" and "nesterov needs" in msg), msg
    # valid values reach the device-pointer check (a host buffer is no device pointer: still refused, with that reason)
    assert lib.ivosw_clamp_sgd(p, p, p, 10, 1e-3, 0.9, 5e-4, 1, 1.0, 1.0, None) == -1
    assert b"not a device pointer" in lib.ivosw_last_error()


def _step_args(p, **over):
    a = dict(n=100, B=4, T=3, gamma=0.95, kind=L.DQN_LOSS_MSE, delta=1.0, lr=1e-3, mu=0.9, wd=0.0, nest=0)
    a.update(over)
    return ([p] * 10 + [a["n"], a["B"], a["T"], a["gamma"], a["kind"], a["delta"]] + [p] * 9 + [1 << 20] +
            [p, a["lr"], a["mu"], a["wd"], a["nest"], 1.0, 1.0, None])


def test_one_call_sgd_step_refuses_bad_arguments(lib):
    keep, p = _fake()
    args = _step_args(p)
    args[0] = None
    assert lib.ivosw_dqn_step_drawn_sgd(*args) == -1 and b"null" in lib.ivosw_last_error()
    args = _step_args(p)
    args[26] = None                                                     # momentum_buf
    assert lib.ivosw_dqn_step_drawn_sgd(*args) == -1 and b"null" in lib.ivosw_last_error()
    for over in (dict(n=0), dict(B=0), dict(T=-1)):
        assert lib.ivosw_dqn_step_drawn_sgd(*_step_args(p, **over)) == -1, over
        assert b"must be positive" in lib.ivosw_last_error()
    assert lib.ivosw_dqn_step_drawn_sgd(*_step_args(p, kind=7)) == -1 and b"loss kind" in lib.ivosw_last_error()
    for (lr, mu, wd, nest), word in BAD:
        assert lib.ivosw_dqn_step_drawn_sgd(*_step_args(p, lr=lr, mu=mu, wd=wd, nest=nest)) == -1, (lr, mu, wd, nest)
        msg = lib.ivosw_last_error().decode()
        assert "ivosw_dqn_step_drawn_sgd" in msg and word in msg, msg
    assert lib.ivosw_dqn_step_drawn_sgd(*_step_args(p, nest=1)) == -1
    assert b"not a device pointer" in lib.ivosw_last_error()


def test_p2p_sgd_refuses_bad_arguments(lib):
    keep, p = _fake()
    table = (ctypes.c_void_p * 2)(p.value, p.value)

    def call(lr=1e-3, mu=0.9, wd=0.0, nest=0, n=64, params=p, buf=p):
        return lib.ivosw_p2p_allreduce_clamp_sgd(p, p, n, 0, 2, table, 1, 100, params, buf, lr, mu, wd, nest, 1.0, None)
    assert call(params=None) == -1 and b"null" in lib.ivosw_last_error()
    assert call(buf=None) == -1 and b"null" in lib.ivosw_last_error()
    assert call(n=0) == -1
    for (lr, mu, wd, nest), word in BAD:
        assert call(lr, mu, wd, nest) == -1, (lr, mu, wd, nest)
        msg = lib.ivosw_last_error().decode()
        assert "ivosw_p2p_allreduce_clamp_sgd" in msg and word in msg, msg
    assert call() == -1 and b"not a device pointer" in lib.ivosw_last_error()


def test_version_marks_the_sgd_entries(lib):
    assert lib.ivosw_version() == 102
