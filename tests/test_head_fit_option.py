"""The head fit without a GPU: the float64 restatement of tests/head_fit_ref.py pinned to REAL torch (nn.Linear in float64, the
reference's loss loop, backward, clamp_, optim.SGD, ExponentialLR), the fixtures' own conditions, option parsing and refusals, the header /
binding / build agreement, and the shipped kernel's resources."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.utils import utils_agent
from tests import head_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("zero_grad", [True, False])
def test_the_float64_restatement_is_torchs_optimiser_loop(zero_grad):
    """3 epochs x 4 steps, torch's own ExponentialLR stepped once per epoch, with and without zero_grad(): w, b and every log row agree
    to 1e-12 relative - the restatement is the reference's optimiser, not a reading of it."""
    feat, target, valid = R.bank(64, 21, invalid=0.2, scale=1.7)
    order = R.draw_order(64, 16, 3, 8)
    rng = np.random.RandomState(2)
    w0, b0 = rng.standard_normal(R.C) * 0.01, -0.25
    lr0, gamma = 6e-4, 0.5
    lr = np.repeat([lr0 * gamma ** e for e in range(3)], 4)              # float64: nothing is rounded to fp32 in this comparison
    tr = []
    log, st = R.run(feat, target, valid, order, lr, 0.9, 5e-4, zero_grad, 0, R.fresh_state(w0, b0, np.float64), np.float64, trace=tr)
    tl, tw, tb, tgw, tgb = R.torch_loop(feat, target, valid, order, None, 0.9, 5e-4, zero_grad, w0, b0, dtype=torch.float64,
                                        scheduler=(lr0, gamma, 4))
    assert order.shape == (12, 16) and st["steps_taken"] == 12 and any(hi or lo for _, hi, lo in tr)      # the clamp takes part
    for got, want in ((log, tl), (st["w"], tw), (st["b"], tb), (st["grad_w"], tgw), (st["grad_b"], tgb)):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (log[:, 2] < 16).any() and (log[:, 2] > 0).all()


def test_fixture_conditions_hold_on_the_reference_alone():
    for zg in (1, 0):
        c, tr = R.clamp_case(), []
        R.run(c["feat"], c["target"], c["valid"], c["order"], c["lr"], c["momentum"], c["weight_decay"], zg, 0, R.fresh_state(c["w0"], c["b0"]),
              np.float64, trace=tr)
        assert any(0.1 * R.C <= hi <= 0.9 * R.C for _, hi, lo in tr) and any(0.1 * R.C <= lo <= 0.9 * R.C for _, hi, lo in tr), tr
    assert c["lr"][0] != c["lr"][-1]                                         # an epoch boundary
    m = R.mixed_case()
    bad = [int((m["valid"][r] == 0).sum()) for r in m["order"]]
    B = m["order"].shape[1]
    assert bad[0] == B and bad[3] == B and all(1 <= v <= B - 1 for i, v in enumerate(bad) if i not in (0, 3))
    assert R.bank(8, 0)[0].min() >= 0


def test_continuation_eval_only_and_all_invalid_steps_in_the_restatement():
    m = R.mixed_case()
    args = (m["feat"], m["target"], m["valid"])
    s0 = R.fresh_state(m["w0"], m["b0"])
    log, st = R.run(*args, m["order"], m["lr"], 0.9, 5e-4, 0, 0, s0)
    la, sa = R.run(*args, m["order"][:2], m["lr"][:2], 0.9, 5e-4, 0, 0, s0)
    lb, sb = R.run(*args, m["order"][2:], m["lr"][2:], 0.9, 5e-4, 0, 0, sa)
    assert np.array_equal(np.concatenate([la, lb]), log) and all(np.array_equal(st[k], sb[k]) for k in st)
    assert np.array_equal(log[0], [0, 0, 0]) and sa["steps_taken"] == 1
    le, se = R.run(*args, m["order"], m["lr"], 0.9, 5e-4, 0, 1, sa)
    assert all(np.array_equal(se[k], sa[k]) for k in sa) and le[1, 2] > 0
    lr = R.lr_table(5e-6, 0.95, 3, 2)
    assert lr.dtype == np.float32 and lr[0] == lr[1] == np.float32(5e-6) and lr[4] == np.float32(5e-6 * 0.95 ** 2)


def _cfg(**kw):
    return {"assess_net": dict(entry.ASSESS_NET_DEFAULTS, **kw)}


def test_option_parsing_and_refusals():
    o = utils_agent.head_fit_options(_cfg())
    assert o == dict(lrs=[5e-6], momentum=0.9, weight_decay=5e-4, gamma=0.95, num_epochs=50, train_batch_size=32, zero_grad=True,
                     augment_copies=1, val_fraction=0.1)                     # the reference's configs/config.yaml
    assert utils_agent.head_fit_options(_cfg(lr=[1e-5, 5e-6], zero_grad=False))["lrs"] == [1e-5, 5e-6]
    assert utils_agent.head_fit_options(dict(entry.ASSESS_NET_DEFAULTS))["num_epochs"] == 50       # the block itself is accepted too
    with pytest.raises(ValueError, match="trunk training is outside this path"):
        utils_agent.head_fit_options(_cfg(fit="all"))
    for bad in (dict(lr=0.0), dict(lr=[]), dict(momentum=1.0), dict(weight_decay=-1.0), dict(gamma=0.0), dict(num_epochs=0),
                dict(augment_copies=0), dict(train_batch_size=257), dict(train_batch_size=0), dict(val_fraction=1.0), dict(zero_grad="maybe")):
        with pytest.raises(ValueError):
            utils_agent.head_fit_options(_cfg(**bad))
    cfg = entry.parse_cli(["with", "assess_net.num_epochs=2", "assess_net.zero_grad=false"], seed=2019, assess_net=dict(entry.ASSESS_NET_DEFAULTS))
    assert cfg.assess_net.num_epochs == 2 and cfg.assess_net.zero_grad is False and cfg.assess_net.lr == 5e-6 and cfg.seed == 2019
    assert "assess_net" not in entry.DEFAULTS                                # the other scripts' keys and defaults stay as they are
    with pytest.raises(SystemExit, match="trunk training is outside this path"):
        entry.main_quality_assessment(["with", "assess_net.fit=trunk"])
    with pytest.raises(SystemExit, match="assess_net.lr"):
        entry.main_quality_assessment(["with", "assess_net.lr=[fast]"])
    assert os.path.exists(os.path.join(ROOT, "quality_assessment.py"))


def test_host_refusals_need_no_gpu():
    from ivos_w_amd.models.assessment import AssessNet
    net = AssessNet()
    with pytest.raises(ValueError, match="2048 weights"):
        net.set_head(torch.zeros(3), torch.zeros(1))
    v0 = net._wver
    net.set_head(torch.full((2048,), 0.5), torch.tensor([0.25]))
    assert net._wver == v0 + 1 and float(net.fc1.weight.detach().min()) == 0.5 and float(net.fc1.bias.detach()) == 0.25
    with pytest.raises(RuntimeError, match="inference-only"):
        net.train().forward_features(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval().forward_features(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8))


def test_argument_errors_do_not_touch_the_gpu():
    lib = L.lib()
    f, i = (ctypes.c_float * 32)(), (ctypes.c_int * 32)()
    assert lib.ivosw_head_fit(None, None, None, 1, None, None, 1, 1, 1, f, f, i, i, *([None] * 8), None) == -1
    assert b"null" in lib.ivosw_last_error()
    assert lib.ivosw_assess_forward_features(None, 1, None, None, 1, 480, 854, None, None, None, 0, 0, None) == -1
    assert lib.ivosw_assess_forward_features_u8(None, 1, None, None, 1, 480, 854, None, None, None, 0, 0, None) == -1
    assert b"features" in lib.ivosw_last_error()


def test_header_binding_build_and_documents_agree():
    header = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for name in ("ivosw_head_fit", "ivosw_assess_forward_features", "ivosw_assess_forward_features_u8"):
        assert name in L.SIGNATURES and name + "(" in header
    assert len(L.SIGNATURES["ivosw_head_fit"][1]) == 22 and len(L.SIGNATURES["ivosw_assess_forward_features"][1]) == 13
    for phrase in ("THE STEP", "a_l = fl(a_l + fl(x[k] * w[k]))", "o = 32, 16, 8, 4, 2, 1", "stored back CLAMPED", "buf = d if steps_taken == 0",
                   "quality_assessment.py:230-270", "#define IVOSW_HEAD_FIT_MAX_FITS 32", "#define IVOSW_HEAD_FIT_MAX_BATCH 256"):
        assert phrase in header, phrase
    assert (L.HEAD_FIT_MAX_FITS, L.HEAD_FIT_MAX_BATCH) == (32, 256)
    from ivos_w_amd import build
    assert "head_fit.hip" in build.SOURCES and build.EXTRA["head_fit.hip"] == ["-ffp-contract=off"]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ivosw_head_fit" in text and "fit_head" in text, doc


def test_the_shipped_kernel_has_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    hits = [r for n, r in kr.kernel_table(L.LIB_PATH).items() if "head_fit_kernel" in n]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spill"] == 0 and hits[0]["vgpr"] <= 128 and hits[0]["lds"] <= 16384, hits
