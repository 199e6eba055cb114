"""The DQN loss option (cfg.agent.loss = "mse" | "huber", cfg.agent.huber_delta) on the host side, no GPU: the CLI carries it to the
agent block, the defaults keep the reference's MSE, the agent refuses what it cannot run, and the C binding declares both _ex entries."""
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry


def test_cli_carries_the_loss_option():
    c = entry.parse_cli(["with", "agent.loss=huber", "agent.huber_delta=0.25"])
    assert (c.agent.loss, c.agent.huber_delta) == ("huber", 0.25)


def test_defaults_are_the_references_mse():
    c = entry.parse_cli([])
    assert (c.agent.loss, c.agent.huber_delta) == ("mse", 1.0)


def test_yaml_config_carries_the_loss_option(tmp_path):
    p = tmp_path / "cfg.yaml"
    p.write_text("agent:\n  loss: huber\n  huber_delta: 0.5\n")
    c = entry.parse_cli(["--config", str(p)])
    assert (c.agent.loss, c.agent.huber_delta) == ("huber", 0.5)
    assert c.agent.gamma == 0.95                                   # the rest of the block keeps its defaults


def test_both_ex_entries_are_bound():
    assert "ivosw_dqn_loss_grad_ex" in L.SIGNATURES and "ivosw_dqn_step_drawn_ex" in L.SIGNATURES
    # the two extra arguments (int loss_kind, float huber_delta) sit right after gamma
    for base in ("ivosw_dqn_loss_grad", "ivosw_dqn_step_drawn"):
        args, ex = L.SIGNATURES[base][1], L.SIGNATURES[base + "_ex"][1]
        g = args.index(L._f)
        assert ex == args[:g + 1] + [L._i, L._f] + args[g + 1:], base
    assert (L.DQN_LOSS_MSE, L.DQN_LOSS_HUBER) == (0, 1)


class AD(dict):
    __getattr__ = dict.__getitem__


def test_agent_reads_the_option_and_refuses_the_unknown():
    from ivos_w_amd.models.agent import Agent
    assert Agent._loss_option(AD(gamma=0.95)) == ("mse", 1.0)        # configs without the keys (bench.py, older tests) stay MSE
    assert Agent._loss_option(AD(loss="huber", huber_delta=0.1)) == ("huber", 0.1)
    assert Agent._loss_option(AD(loss="huber", huber_delta=2)) == ("huber", 2.0)
    for bad in (dict(loss="l1"), dict(loss="Huber"), dict(loss="huber", huber_delta=0), dict(loss="huber", huber_delta=-1.0),
                dict(loss="huber", huber_delta=float("nan")), dict(loss="huber", huber_delta=float("inf")),
                dict(loss="huber", huber_delta=1e39), dict(loss="huber", huber_delta="0.5"), dict(loss="huber", huber_delta=True)):
        with pytest.raises(ValueError):
            Agent._loss_option(AD(bad))
