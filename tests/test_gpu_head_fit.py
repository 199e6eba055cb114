"""GPU: ivosw_head_fit through the C ABI against tests/head_fit_ref.py on synthetic non-negative feature banks (M <= 512).

Tolerance (the project's rule from the BPTT test, head_fit_ref.within): the device's error against the float64 restatement on w, b and the
log is at most 2 x the error of the same loop written with real torch in fp32 on the CPU, or 1e-6 of the tensor's scale, whichever is
larger.  Determinism, continuation and the untouched-state cases compare bits."""
import ctypes

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from tests import head_fit_ref as R

pytestmark = pytest.mark.gpu
C = R.C
KEYS = ("w", "b", "buf_w", "buf_b", "grad_w", "grad_b")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def device_fit(dev, feat, target, valid, orders, lrs, momentum, weight_decay, zero_grad, eval_only, states):
    """One ivosw_head_fit launch of len(states) fits; per-fit lists throughout.  -> (logs [n_fits,n_steps,3] numpy, new states)."""
    k = len(states)
    order = np.stack([np.asarray(o, dtype=np.int32) for o in orders])
    n_steps, B = order.shape[1:]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    d_feat, d_tgt, d_val = t(feat, np.float32), t(target, np.float32), t(valid, np.uint8)
    d_order, d_lr = t(order, np.int32), t(np.stack(lrs), np.float32)
    d = {key: t(np.stack([np.asarray(s[key], dtype=np.float32).reshape(-1) for s in states]), np.float32) for key in KEYS}
    d_taken = t([s["steps_taken"] for s in states], np.int32)
    d_log = torch.full((k, n_steps, 3), -7.0, dtype=torch.float32, device=dev)
    f_arr = lambda v: (ctypes.c_float * k)(*[float(x) for x in v])
    rc = L.lib().ivosw_head_fit(L.dptr(d_feat), L.dptr(d_tgt), L.dptr(d_val), len(feat), L.dptr(d_order), L.dptr(d_lr), k, n_steps, B,
                                f_arr(momentum), f_arr(weight_decay), L.int_array(zero_grad), L.int_array(eval_only),
                                *[L.dptr(d[key]) for key in KEYS], L.dptr(d_taken), L.dptr(d_log), L.stream_ptr(dev))
    L.check(rc, "head_fit")
    torch.cuda.synchronize(dev)
    taken = d_taken.cpu().numpy()
    out = []
    for i in range(k):
        s = {key: d[key][i].cpu().numpy().copy() for key in KEYS}
        for key in ("b", "buf_b", "grad_b"):
            s[key] = np.float32(s[key][0])
        s["steps_taken"] = int(taken[i])
        out.append(s)
    return d_log.cpu().numpy(), out


def one(dev, case, zero_grad=1, eval_only=0, state=None, order=None, lr=None, momentum=None):
    state = R.fresh_state(case["w0"], case["b0"]) if state is None else state
    logs, states = device_fit(dev, case["feat"], case["target"], case["valid"], [case["order"] if order is None else order],
                              [case["lr"] if lr is None else lr], [case["momentum"] if momentum is None else momentum],
                              [case["weight_decay"]], [zero_grad], [eval_only], [state])
    return logs[0], states[0]


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.float32).view(np.uint32), np.asarray(b[k], dtype=np.float32).view(np.uint32))
               for k in KEYS) and a["steps_taken"] == b["steps_taken"]


_refs = {}


def refs(name, case, zero_grad=1, momentum=None):
    """(float64 log, float64 state, fp32 numpy log, fp32 numpy state, torch-fp32 loop) of a case from a fresh state, computed once."""
    key = (name, zero_grad, momentum)
    if key not in _refs:
        mom = case["momentum"] if momentum is None else momentum
        args = (case["feat"], case["target"], case["valid"], case["order"], case["lr"], mom, case["weight_decay"], zero_grad)
        l64, s64 = R.run(*args, 0, R.fresh_state(case["w0"], case["b0"]), np.float64)
        l32, s32 = R.run(*args, 0, R.fresh_state(case["w0"], case["b0"]), np.float32)
        _refs[key] = (l64, s64, l32, s32, R.torch_loop(*args, case["w0"], case["b0"]))
    return _refs[key]


def check_against_refs(name, log, st, ref, grads=False):
    l64, s64, l32, s32, (tl, tw, tb, tgw, tgb) = ref
    R.within(log, l64, tl, name + " log")
    R.within(st["w"], s64["w"], tw, name + " w")
    R.within(st["b"], s64["b"], tb, name + " b")
    if grads:
        R.within(st["grad_w"], s64["grad_w"], tgw, name + " grad_w")
        R.within(st["grad_b"], s64["grad_b"], tgb, name + " grad_b")
    assert st["steps_taken"] == s64["steps_taken"]
    # the fp32 restatement states the device's operation order: the same bits
    assert np.array_equal(log.view(np.uint32), l32.view(np.uint32)), name
    assert same_bits(st, s32), name


def batch_case(B):
    """2 epochs (an epoch boundary in lr), momentum 0.9, weight decay; M = 2 B + 3 rows (B = 256: M = 515 would pass 512, so 2 x 256)."""
    M = 512 if B == 256 else max(2 * B + 3, 8)
    feat, target, valid = R.bank(M, 100 + B)
    steps = M // B if B > 1 else 3
    order = R.draw_order(M, B, 2, B)
    if B == 1:
        order = np.concatenate([order[:3], order[M:M + 3]])
    rng = np.random.RandomState(B)
    return dict(feat=feat, target=target, valid=valid, order=order, lr=R.lr_table(2e-4, 0.5, 2, steps), momentum=0.9, weight_decay=5e-4,
                w0=(rng.standard_normal(C) * 0.01).astype(np.float32), b0=0.05)


@pytest.mark.parametrize("B", [1, 17, 32, 256])
def test_batch_sizes_momentum_weight_decay_and_an_epoch_boundary(dev, B):
    case = batch_case(B)
    assert case["lr"][0] != case["lr"][-1] and case["order"].shape[1] == B
    log, st = one(dev, case)
    check_against_refs(f"B={B}", log, st, refs(f"B{B}", case))


def test_momentum_zero(dev):
    case = batch_case(17)
    log, st = one(dev, case, momentum=0.0)
    check_against_refs("momentum=0", log, st, refs("B17", case, momentum=0.0))
    assert not np.array_equal(st["w"], one(dev, case)[1]["w"])


def test_mixed_validity_and_steps_with_every_row_invalid(dev):
    case = R.mixed_case()
    bad = [int((case["valid"][r] == 0).sum()) for r in case["order"]]
    assert bad[0] == 17 and bad[3] == 17 and all(1 <= v <= 16 for i, v in enumerate(bad) if i not in (0, 3))
    log, st = one(dev, case)
    check_against_refs("mixed", log, st, refs("mixed", case))
    assert np.array_equal(log[0], [0, 0, 0]) and np.array_equal(log[3], [0, 0, 0]) and st["steps_taken"] == 4
    # only invalid rows: nothing at all changes, and the next step is still the first
    s0 = R.fresh_state(case["w0"], case["b0"])
    s0["grad_w"][:] = 0.25
    s0["buf_w"][:] = -0.5
    log1, s1 = one(dev, case, state=s0, order=case["order"][[0, 3]], lr=case["lr"][:2], zero_grad=0)
    assert np.array_equal(log1, np.zeros((2, 3), np.float32)) and same_bits(s0, s1) and s1["steps_taken"] == 0
    log2, s2 = one(dev, case, state=s1, order=case["order"][1:2], lr=case["lr"][1:2])
    want_log, want = R.run(case["feat"], case["target"], case["valid"], case["order"][1:2], case["lr"][1:2], 0.9, 5e-4, 1, 0, s0, np.float32)
    assert same_bits(s2, want) and np.array_equal(log2, want_log)
    assert np.array_equal(want["buf_w"], (want["grad_w"] + np.float32(5e-4) * s0["w"]).astype(np.float32))      # first step: buf = d, the old buffer is gone


@pytest.mark.parametrize("zero_grad", [1, 0])
def test_clamp_engaged_on_both_sides_with_and_without_zero_grad(dev, zero_grad):
    case = R.clamp_case()
    log, st = one(dev, case, zero_grad=zero_grad)
    check_against_refs(f"clamp zero_grad={zero_grad}", log, st, refs("clamp", case, zero_grad=zero_grad), grads=True)
    assert np.abs(st["grad_w"]).max() <= 1.0
    other = refs("clamp", case, zero_grad=1 - zero_grad)[1]
    assert not np.allclose(st["grad_w"], other["grad_w"], atol=1e-3)


def test_a_continued_call_equals_one_call_bit_for_bit(dev):
    case = R.clamp_case()
    for zg in (1, 0):
        log, st = one(dev, case, zero_grad=zg)
        la, sa = one(dev, case, zero_grad=zg, order=case["order"][:3], lr=case["lr"][:3])
        lb, sb = one(dev, case, zero_grad=zg, order=case["order"][3:], lr=case["lr"][3:], state=sa)
        assert sa["steps_taken"] == 3 and same_bits(st, sb)
        assert np.array_equal(np.concatenate([la, lb]).view(np.uint32), log.view(np.uint32))


def test_eval_only_leaves_all_state_unchanged(dev):
    case = R.mixed_case()
    _, s0 = one(dev, case, order=case["order"][:3], lr=case["lr"][:3])
    log, s1 = one(dev, case, state=s0, eval_only=1)
    assert same_bits(s0, s1)
    want, _ = R.run(case["feat"], case["target"], case["valid"], case["order"], case["lr"], 0.9, 5e-4, 1, 1, s0, np.float32)
    assert np.array_equal(log.view(np.uint32), want.view(np.uint32))
    want64, _ = R.run(case["feat"], case["target"], case["valid"], case["order"], case["lr"], 0.9, 5e-4, 1, 1, s0, np.float64)
    assert np.abs(log - want64).max() <= 1e-5 * np.abs(want64).max()


def test_runs_and_launch_positions_give_the_same_bits_and_32_fits_differ(dev):
    case = batch_case(32)
    log, st = one(dev, case)
    log_again, st_again = one(dev, case)
    assert same_bits(st, st_again) and np.array_equal(log.view(np.uint32), log_again.view(np.uint32))
    # 32 fits with their own rates and index tables; members 0, 13 and 31 are the fit above
    steps = case["order"].shape[0]
    lrs = [R.lr_table(2e-4 * (1 + 0.25 * k), 0.5, 2, steps // 2) for k in range(32)]
    orders = [R.draw_order(len(case["feat"]), 32, 2, 1000 + k) for k in range(32)]
    moms = [0.9 if k % 2 == 0 else 0.5 for k in range(32)]
    for k in (0, 13, 31):
        lrs[k], orders[k], moms[k] = case["lr"], case["order"], 0.9
    fresh = [R.fresh_state(case["w0"], case["b0"]) for _ in range(32)]
    logs, states = device_fit(dev, case["feat"], case["target"], case["valid"], orders, lrs, moms, [5e-4] * 32, [1] * 32, [0] * 32, fresh)
    for k in (0, 13, 31):
        assert same_bits(states[k], st) and np.array_equal(logs[k].view(np.uint32), log.view(np.uint32)), k
    # ... and 32 fits that differ in lr alone give 32 different results, each within tolerance of its own reference
    lrs = [R.lr_table(2e-4 * (1 + 0.25 * k), 0.5, 2, steps // 2) for k in range(32)]
    logs, states = device_fit(dev, case["feat"], case["target"], case["valid"], [case["order"]] * 32, lrs, [0.9] * 32, [5e-4] * 32, [1] * 32,
                              [0] * 32, fresh)
    assert len({states[k]["w"].tobytes() for k in range(32)}) == 32
    for k in range(32):
        c = dict(case, lr=lrs[k])
        check_against_refs(f"fit {k} of 32", logs[k], states[k], refs(f"sweep{k}", c))


def test_argument_errors_return_without_a_launch(dev):
    lib = L.lib()
    z = torch.zeros(4096, dtype=torch.float32, device=dev)
    zi = torch.zeros(64, dtype=torch.int32, device=dev)
    zb = torch.ones(64, dtype=torch.uint8, device=dev)
    log = torch.full((8,), -7.0, dtype=torch.float32, device=dev)
    one_f, one_i = (ctypes.c_float * 32)(), (ctypes.c_int * 32)()

    def call(feat=z, target=z, valid=zb, M=2, order=zi, lr=z, n_fits=1, n_steps=1, B=2, mom=one_f, wd=one_f, zg=one_i, ev=one_i, w=z, b=z,
             buf_w=z, buf_b=z, grad_w=z, grad_b=z, taken=zi, out=log):
        p = lambda v: None if v is None else (v if not isinstance(v, torch.Tensor) else L.dptr(v))
        return lib.ivosw_head_fit(p(feat), p(target), p(valid), M, p(order), p(lr), n_fits, n_steps, B, p(mom), p(wd), p(zg), p(ev), p(w), p(b),
                                  p(buf_w), p(buf_b), p(grad_w), p(grad_b), p(taken), p(out), L.stream_ptr(dev))
    for name in ("feat", "target", "valid", "order", "lr", "mom", "wd", "zg", "ev", "w", "b", "buf_w", "buf_b", "grad_w", "grad_b", "taken", "out"):
        assert call(**{name: None}) == -1 and b"null" in lib.ivosw_last_error(), name
    for kw, word in ((dict(B=0), b"B outside"), (dict(B=257), b"B outside"), (dict(n_fits=0), b"n_fits"), (dict(n_fits=33), b"n_fits"),
                     (dict(M=0), b"M must"), (dict(n_steps=0), b"n_steps")):
        assert call(**kw) == -1 and word in lib.ivosw_last_error(), kw
    torch.cuda.synchronize(dev)
    assert float(log.min()) == -7.0 and float(z.abs().max()) == 0.0 and int(zi.abs().max()) == 0
