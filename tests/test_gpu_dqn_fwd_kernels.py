"""The Brain's forward kernels - enc_fused_kernel, dec_fused_kernel (csrc/brain_fused.h), lstm_fwd_kernel<1|2|4>, lstm_fwd_quad_kernel<1|2|4>,
lstm_fwd_mfma_kernel, lstm_fwd_mfma_pair_kernel, lstm_fwd_quad_ragged_kernel and brain_fwd_mega_kernel (csrc/lstm_fwd.h) - each ALONE through
its probe entry (include/ivosw_probe.h, libivosw_probe.so) on tensors this file makes, against the float64 restatements of tests/dqn_ref.py
(pinned to the oracle on the CPU by tests/test_dqn_ref.py).  The rules and helpers are those of tests/test_gpu_dqn_kernels.py:

  reach   every kernel form, the two-job launches and the product's own choice of form ran in a case of their own
  exact   small-integer operands whose sums no fp32 order can change: the output equals float64, zero tolerance; what one launch writes
          equals bit for bit what another launch of the same arithmetic writes (a job of a pair alone, a ragged slice as a batch of one,
          the mega kernel's recurrence as the MFMA form's); hprev IS hs of the frame before, bit for bit
  dense   random operands: per element within (K + 2) 2^-23 sum |a||b| per stage, the previous stage's bound carried through |W|
          (dqn_ref.enc_bounds, dec_bounds)
  step    every step of the recurrence from the device's OWN hprev and previous c: gates, c and h within dqn_ref.step_bounds of lstm_step
          in float64 - the K = 128 term through the activation's slope plus 4 x the error of the fp32 numpy restatement of the device's
          activation expressions on the fixture's pre-activations (v_exp_f32, v_rcp_f32 may each be an ulp off)
  chain   hs from a zero state against lstm_fwd in float64: max(2 x the fp32 numpy restatement's error, 1e-6) of the largest element
  guards  every output sits between guard rows of a NaN pattern that must stay, rows that are not kept hold it too; every row-indexed
          operand is followed by NaN guard rows (the kernels clamp tail reads to the last live row)
  refuse  what a kernel does not take is refused and nothing is written

Measured figures: LAB_NOTES.md, "Brain forward kernels alone"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from tests import dqn_ref as R
from tests.test_gpu_dqn_kernels import GUARD, NAN32, _ok, _op, _out, _ratio, _read, _refused, _same, _untouched

pytestmark = pytest.mark.gpu

REACHED = set()
NPAD = 512              # rows of the refusal test's stand-in operand: 512 x 512 floats hold an arena and every operand of its shapes
WORST = {}              # form -> [gates, c, h, chain / allowed]: the worst ratios any case of this run saw


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows_op(a, cols, dev):
    """_op for an operand that may have no rows at all (then the buffer is guard rows only)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, cols)
    host = np.full((a.shape[0] + GUARD, cols), NAN32, np.int32)
    host[:a.shape[0]] = a.view(np.int32)
    buf = torch.from_numpy(host).to(dev)
    return buf, L.dptr(buf)


def _parr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[None if p is None else p.value for p in ptrs])


def _kept(buf, rows, first, what):
    """The rows [first, rows) of an output whose rows below `first` are not written: they and the guards must hold the pattern."""
    got, clean = _read(buf, rows)
    assert clean, f"{what}: a guard row was written"
    assert (got[:first].view(np.int32) == NAN32).all(), f"{what}: a row below the first kept row was written"
    assert np.isfinite(got[first:]).all(), f"{what}: a kept row was not written, or a guard row of an operand reached it"
    return got[first:]


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int32) for a in arrays]


def _bit_equal(a, b, what):
    for i, (x, y) in enumerate(zip(_bits(*a), _bits(*b))):
        assert np.array_equal(x, y), f"{what}: output {i} differs in {int((x != y).sum())} of {x.size} elements"


@functools.lru_cache(maxsize=None)
def _params(seed, exact):
    return R.brain_params(seed, exact)


# ---------------------------------------------------------------- encoder
def _enc(dev, jobs):
    """jobs: (P, x, rows0, keep_row) each -> [(gx, a1 kept rows, e kept rows)] of ONE launch."""
    lib = L.probe_lib()
    ops = [(_op(R.arena(P)[:, None], dev), _rows_op(x[:r0], 2, dev), _rows_op(x[r0:], 2, dev)) for P, x, r0, _ in jobs]
    outs = [(_out(x.shape[0], 512, dev), _out(x.shape[0], 128, dev), _out(x.shape[0], 128, dev)) for _, x, _, _ in jobs]
    col = lambda src, i: _parr([s[i][1] for s in src])
    rc = lib.ivosw_enc_fused_probe(len(jobs), col(ops, 0), col(ops, 1), col(ops, 2), L.int_array([j[2] for j in jobs]),
                                   L.int_array([j[1].shape[0] for j in jobs]), L.int_array([j[3] for j in jobs]), col(outs, 0), col(outs, 1),
                                   col(outs, 2), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("enc" if len(jobs) == 1 else "enc x2")
    res = []
    for (_, x, _, keep_row), o in zip(jobs, outs):
        rows = x.shape[0]
        res.append((_kept(o[0][0], rows, 0, "gx"), _kept(o[1][0], rows, keep_row, "a1"), _kept(o[2][0], rows, keep_row, "e")))
    return res


@pytest.mark.parametrize("rows", R.ENC_ROWS)
def test_enc_exact_fixture_is_bit_equal_to_fp64_and_keeps_only_the_kept_rows(dev, rows):
    """Integer operands: gx of every row, a1 and e of the rows [keep_row, rows) equal float64; below keep_row the pattern stays.  Every
    position of the x / x2 boundary and of keep_row of dqn_ref.enc_cases."""
    P, x = _params(0, True), R.enc_fixture(rows, True)
    a1, e, gx = R.enc(P, x)
    for rows0, keep_row in R.enc_cases(rows):
        (ggx, ga1, ge), = _enc(dev, [(P, x, rows0, keep_row)])
        what = f"rows0={rows0} keep_row={keep_row}"
        _same(ggx, gx, "gx " + what)
        _same(ga1, a1[keep_row:], "a1 " + what)
        _same(ge, e[keep_row:], "e " + what)


@pytest.mark.parametrize("rows", R.ENC_ROWS)
def test_enc_dense_fixture_is_within_its_derived_three_stage_bound(dev, rows):
    """a1, e and gx within dqn_ref.enc_bounds of float64; the units whose pre-activation IS +-x pass +0, -0 and the subnormals through the
    relu exactly (their bound is 4 x 2^-23 of a subnormal)."""
    P, x = _params(0, False), R.enc_fixture(rows, False)
    a1, e, gx = R.enc(P, x)
    b_a1, b_e, b_gx = R.enc_bounds(P, x)
    worst = [0.0, 0.0, 0.0]
    for rows0, keep_row in R.enc_cases(rows):
        (ggx, ga1, ge), = _enc(dev, [(P, x, rows0, keep_row)])
        r = (_ratio(ga1, a1[keep_row:], b_a1[keep_row:]) if keep_row < rows else 0.0,
             _ratio(ge, e[keep_row:], b_e[keep_row:]) if keep_row < rows else 0.0, _ratio(ggx, gx, b_gx))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1.0, f"rows0={rows0} keep_row={keep_row}: a1, e, gx are {r} x their bounds"
        if keep_row < rows:
            assert np.array_equal(ga1[:, :4].astype(np.float64), a1[keep_row:, :4]), "the relu at its edge"
    print(f"\nFIG enc rows {rows}: worst |.-ref64| / bound a1 {worst[0]:.3f}, e {worst[1]:.3f}, gx {worst[2]:.3f}")


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "dense"))
def test_enc_two_jobs_with_different_arenas_each_equal_their_single_launch(dev, exact):
    """Job 0: 49 rows (x2 from row 1, kept from row 48), job 1: 47 rows of ANOTHER net (no x2, all kept) behind it in one launch: either
    job's outputs are bit for bit those of its own single launch, and with the integer fixture equal to float64."""
    jobs = [(_params(i, exact), R.enc_fixture(rows, exact, i), rows0, keep) for i, (rows, rows0, keep) in enumerate(R.TWO_JOBS)]
    both = _enc(dev, jobs)
    for i, job in enumerate(jobs):
        _bit_equal(both[i], _enc(dev, [job])[0], f"job {i}")
        if exact:
            a1, e, gx = R.enc(job[0], job[1])
            _same(both[i][0], gx, f"gx of job {i}")
            _same(both[i][1], a1[job[3]:], f"a1 of job {i}")
            _same(both[i][2], e[job[3]:], f"e of job {i}")
    assert not np.array_equal(R.arena(jobs[0][0]), R.arena(jobs[1][0]))


# ---------------------------------------------------------------- decoder
def _dec(dev, jobs):
    """jobs: (P, hs, keep_row) each -> [(q [rows], d1 kept rows)] of ONE launch."""
    lib = L.probe_lib()
    ops = [(_op(R.arena(P)[:, None], dev), _op(hs, dev)) for P, hs, _ in jobs]
    outs = [(_out(hs.shape[0], 128, dev), _out(hs.shape[0], 1, dev)) for _, hs, _ in jobs]
    col = lambda src, i: _parr([s[i][1] for s in src])
    rc = lib.ivosw_dec_fused_probe(len(jobs), col(ops, 0), col(ops, 1), L.int_array([j[1].shape[0] for j in jobs]),
                                   L.int_array([j[2] for j in jobs]), col(outs, 0), col(outs, 1), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("dec" if len(jobs) == 1 else "dec x2")
    return [(_kept(o[1][0], hs.shape[0], 0, "q")[:, 0], _kept(o[0][0], hs.shape[0], keep, "d1")) for (_, hs, keep), o in zip(jobs, outs)]


def _keep_rows(rows):
    return sorted(k for k in {0, 50, rows} if k <= rows)


@pytest.mark.parametrize("rows", R.ENC_ROWS)
def test_dec_exact_fixture_is_bit_equal_to_fp64_and_keeps_only_the_kept_rows(dev, rows):
    P, hs = _params(0, True), R.dec_fixture(rows, True)
    d1, q = R.dec(P, hs)
    for keep_row in _keep_rows(rows):
        (gq, gd1), = _dec(dev, [(P, hs, keep_row)])
        _same(gq, q, f"q keep_row={keep_row}")
        _same(gd1, d1[keep_row:], f"d1 keep_row={keep_row}")


@pytest.mark.parametrize("rows", R.ENC_ROWS)
def test_dec_dense_fixture_is_within_its_derived_two_stage_bound(dev, rows):
    """d1 within the K = 256 bound, q within K = 128 on the kernel's d1 plus d1's bound through |w4| (dqn_ref.dec_bounds); hs carries +0, -0,
    negatives, the smallest subnormal and positives in every row."""
    P, hs = _params(0, False), R.dec_fixture(rows, False)
    d1, q = R.dec(P, hs)
    b_d1, b_q = R.dec_bounds(P, hs)
    worst = [0.0, 0.0]
    for keep_row in _keep_rows(rows):
        (gq, gd1), = _dec(dev, [(P, hs, keep_row)])
        r = (_ratio(gd1, d1[keep_row:], b_d1[keep_row:]) if keep_row < rows else 0.0, _ratio(gq, q, b_q))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1.0, f"keep_row={keep_row}: d1, q are {r} x their bounds"
    print(f"\nFIG dec rows {rows}: worst |.-ref64| / bound d1 {worst[0]:.3f}, q {worst[1]:.3f}")


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "dense"))
def test_dec_two_jobs_with_different_arenas_each_equal_their_single_launch(dev, exact):
    jobs = [(_params(i, exact), R.dec_fixture(rows, exact, i), keep) for i, (rows, _, keep) in enumerate(R.TWO_JOBS)]
    both = _dec(dev, jobs)
    for i, job in enumerate(jobs):
        _bit_equal(both[i], _dec(dev, [job])[0], f"job {i}")
        if exact:
            d1, q = R.dec(job[0], job[1])
            _same(both[i][0], q, f"q of job {i}")
            _same(both[i][1], d1[job[2]:], f"d1 of job {i}")


# ---------------------------------------------------------------- recurrence
class Fwd:
    """What one recurrence launch left: hs [N,T,256] and, for the samples >= keep_from, gates [2,Nk,T,512], cs, hprev [2,Nk,T,128]."""


def _rec_bufs(dev, N, T, keep_from, kept):
    Nk = N - keep_from
    hs = _out(N * T, 256, dev)
    if not kept or Nk == 0:
        return hs, None, None, None
    return hs, _out(2 * Nk * T, 512, dev), _out(2 * Nk * T, 128, dev), _out(2 * Nk * T, 128, dev)


def _rec_read(bufs, N, T, keep_from, hs_from=0):
    o = Fwd()
    Nk = N - keep_from
    o.hs = _kept(bufs[0][0], N * T, hs_from * T, "hs").reshape(N - hs_from, T, 256)
    o.gates = o.cs = o.hprev = None
    if bufs[1] is not None:
        o.gates = _kept(bufs[1][0], 2 * Nk * T, 0, "gates").reshape(2, Nk, T, 512)
        o.cs = _kept(bufs[2][0], 2 * Nk * T, 0, "cs").reshape(2, Nk, T, 128)
        o.hprev = _kept(bufs[3][0], 2 * Nk * T, 0, "hprev").reshape(2, Nk, T, 128)
    return o


def _p(b):
    return None if b is None else b[1]


def _lstm(dev, whh, gx, keep_from, form, kept=True):
    lib = L.probe_lib()
    N, T, _ = gx.shape
    (kw, pw), (kg, pg) = _op(whh, dev), _op(gx.reshape(N * T, 512), dev)
    bufs = _rec_bufs(dev, N, T, keep_from, kept)
    ran = ctypes.c_int(-1)
    rc = lib.ivosw_lstm_fwd_probe(pw, pg, _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), N, T, keep_from, form, ctypes.byref(ran),
                                  L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    assert ran.value == form or (form == 0 and ran.value in R.FORM_NAMES)
    REACHED.add(R.FORM_NAMES[ran.value] if form else "auto")
    o = _rec_read(bufs, N, T, keep_from)
    o.ran = ran.value
    return o


@functools.lru_cache(maxsize=None)
def _chain(N, T, seed=0):
    """The fixture, its float64 chain, the fp32 restatement's error and the activation terms: computed once per shape."""
    whh, gx = R.fwd_fixture(N, T, seed)
    hs = R.lstm_fwd(whh, gx)[0]
    e32 = R.rel_err(R.lstm_fwd(whh, gx, np.float32)[0], hs)
    return whh, gx, hs, max(2 * e32, 1e-6), R.act_terms(whh, gx)


def _links(o, N, T, keep_from, what):
    """(a): hprev is hs of the frame the direction consumed before, bit for bit, and zero at its first frame; at T = 1 both directions' gates
    are the activation of gx alone."""
    if o.gates is None:
        return
    for d in range(2):
        h = o.hs[keep_from:, :, d * 128:(d + 1) * 128]
        first = 0 if d == 0 else T - 1
        assert not o.hprev[d, :, first].any(), f"{what}: hprev of direction {d} is not zero at its first frame"
        if T > 1:
            prev, cur = (h[:, :-1], o.hprev[d, :, 1:]) if d == 0 else (h[:, 1:], o.hprev[d, :, :-1])
            assert np.array_equal(*_bits(prev, cur)), f"{what}: hprev of direction {d} is not hs of the frame before"
    if T == 1:
        assert np.array_equal(*_bits(o.gates[0], o.gates[1])) and np.array_equal(*_bits(o.cs[0], o.cs[1])), f"{what}: T = 1, the directions differ"


def _steps(o, whh, gx, keep_from, acts):
    """(b): worst |device - lstm_step in float64| / allowance over the kept steps, for gates, c and h."""
    if o.gates is None:
        return 0.0, 0.0, 0.0
    T = gx.shape[1]
    cprev = np.zeros_like(o.cs)
    if T > 1:
        cprev[0, :, 1:], cprev[1, :, :-1] = o.cs[0, :, :-1], o.cs[1, :, 1:]
    gxk = np.broadcast_to(gx[keep_from:][None], o.gates.shape)
    g, c, h = R.lstm_step(whh, gxk, o.hprev, cprev)
    b_g, b_c, b_h = R.step_bounds(whh, gxk, o.hprev, cprev, acts)
    hk = np.stack([o.hs[keep_from:, :, :128], o.hs[keep_from:, :, 128:]])
    return _ratio(o.gates, g, b_g), _ratio(o.cs, c, b_c), _ratio(hk, h, b_h)


def _hold(o, N, T, keep_from, form, seed=0, what=""):
    """Layers (a), (b) and (c) on one launch's outputs; the figures go into WORST."""
    whh, gx, ref, allowed, acts = _chain(N, T, seed)
    what = what or f"{R.FORM_NAMES[form]} N={N} T={T} keep_from={keep_from}"
    _links(o, N, T, keep_from, what)
    rg, rc, rh = _steps(o, whh, gx, keep_from, acts)
    err = R.rel_err(o.hs, ref)
    w = WORST.setdefault(R.FORM_NAMES[form], [0.0, 0.0, 0.0, 0.0])
    WORST[R.FORM_NAMES[form]] = [max(a, b) for a, b in zip(w, (rg, rc, rh, err / allowed))]
    assert max(rg, rc, rh) <= 1.0, f"{what}: a step's gates, c, h are {rg:.3f}, {rc:.3f}, {rh:.3f} x their allowances"
    assert err <= allowed, f"{what}: hs is {err:.3e} from the float64 chain, allowed {allowed:.3e}"
    return rg, rc, rh, err, allowed


def _act_alone(o, gx, acts):
    """T = 1: h is zero, the pre-activation IS gx (fma(0, w, a) == a), so the gates' whole error is the activation's.  A figure for the
    notes (the step check above is the assertion): worst error / ACT_MARGIN-fold restatement error, sigmoid gates and g gate."""
    pre = np.broadcast_to(gx[None].astype(np.float64), o.gates.shape)
    err = np.abs(o.gates.astype(np.float64) - R.lstm_step(np.zeros((512, 128)), pre, np.zeros(o.hprev.shape), np.zeros(o.cs.shape))[0])
    return float(np.delete(err, np.s_[256:384], -1).max() / acts[0]), float(err[..., 256:384].max() / acts[1])


def _forms_at(dev, N, T, forms):
    whh, gx, _, _, acts = _chain(N, T)
    for form in forms:
        first = None
        for keep_from in sorted({0, 1, N}):
            o = _lstm(dev, whh, gx, keep_from, form)
            assert (o.gates is None) == (keep_from == N)
            rg, rc, rh, err, allowed = _hold(o, N, T, keep_from, form)
            if first is None:
                first = o
                if T == 1:
                    print("\nFIG lstm_fwd %s N %d T 1: activation error alone, sigmoid %.3f, tanh %.3f of the activation terms" %
                          ((R.FORM_NAMES[form], N) + _act_alone(o, gx, acts)))
                print(f"\nFIG lstm_fwd {R.FORM_NAMES[form]} N {N} T {T}: step gates {rg:.3f}, c {rc:.3f}, h {rh:.3f} of their allowances; "
                      f"chain {err:.3e}, allowed {allowed:.3e}")
                continue
            _bit_equal([o.hs], [first.hs], f"{R.FORM_NAMES[form]} N={N} T={T}: hs at keep_from={keep_from} and 0")
            if o.gates is not None:                          # the kept rows are those of keep_from = 0, indexed from keep_from
                _bit_equal([o.gates, o.cs, o.hprev], [first.gates[:, keep_from:], first.cs[:, keep_from:], first.hprev[:, keep_from:]],
                           f"{R.FORM_NAMES[form]} N={N} T={T} keep_from={keep_from}")


@pytest.mark.parametrize("N,T", [(N, T) for N in R.FWD_N_SMALL for T in R.FWD_T])
def test_lstm_fwd_plain_and_quad_forms_link_step_and_chain(dev, N, T):
    """lstm_fwd_kernel<1|2|4> and lstm_fwd_quad_kernel<1|2|4>: N = 3 is six rows - a two-row tail and a workgroup across the direction
    boundary at R = 4 -; keep_from 0, 1 and N (nothing kept, NULL pointers).  What is kept does not depend on keep_from, hs not at all."""
    _forms_at(dev, N, T, R.FWD_FORMS_SMALL)


@pytest.mark.parametrize("N,T", [(N, T) for N in R.FWD_N_MFMA for T in R.FWD_T])
def test_lstm_fwd_mfma_form_links_steps_and_chain(dev, N, T):
    """lstm_fwd_mfma_kernel: a full grid (N = 4), a tail of two rows (5), a workgroup across the direction boundary (5, 6)."""
    _forms_at(dev, N, T, (R.FORM_MFMA,))


@pytest.mark.parametrize("N,forms", [(3, R.FWD_FORMS_SMALL), (5, (R.FORM_MFMA,))], ids=("plain+quad", "mfma"))
def test_lstm_fwd_saturated_gates_are_exactly_0_1_and_pm1(dev, N, forms):
    """gx = +-100 in every combination of gate signs: exp2 overflows or vanishes beside 1, so i, f, o are exactly 0 or 1 and g exactly +-1,
    and every output is finite."""
    T = 9
    whh, gx = R.saturating_fixture(N, T)
    want = np.round(R.lstm_fwd(whh, gx)[1])
    assert set(np.unique(want[..., :256])) == {0.0, 1.0} and set(np.unique(want[..., 256:384])) == {-1.0, 1.0}
    for form in forms:
        o = _lstm(dev, whh, gx, 0, form)                   # (_kept: every output is finite)
        _same(o.gates, want, f"{R.FORM_NAMES[form]}: saturated gates")
        assert np.abs(o.cs).max() <= T and np.abs(o.hs).max() <= 1.0


@pytest.mark.parametrize("N", (3, 4, 130))
def test_lstm_fwd_auto_is_the_products_choice_of_form(dev, N):
    T = 2
    whh, gx, _, _, _ = _chain(N, T)
    o = _lstm(dev, whh, gx, 0, 0)
    assert o.ran == R.product_form(N), "the probe's own choice is not the forward drivers' rule"
    _hold(o, N, T, 0, o.ran, what=f"auto N={N}")
    if N == 130:                                             # 260 rows: 65 workgroups, both halves of the batch
        _bit_equal([o.hs[:5]], [_lstm(dev, whh, gx[:5], 5, R.FORM_MFMA).hs], "rows of a large batch against the same rows alone")


def test_lstm_fwd_pair_jobs_each_equal_their_single_launch(dev):
    """lstm_fwd_mfma_pair_kernel: (N = 5, kept from sample 2) and (N = 4, nothing kept) with different W_hh in one launch."""
    lib = L.probe_lib()
    T = 9
    jobs = [(5, 2, True, 0), (4, 4, False, 1)]
    ops, bufs = [], []
    for N, keep_from, kept, seed in jobs:
        whh, gx, _, _, _ = _chain(N, T, seed)
        ops.append((_op(whh, dev), _op(gx.reshape(N * T, 512), dev)))
        bufs.append(_rec_bufs(dev, N, T, keep_from, kept))
    col = lambda src, i: _parr([_p(s[i]) for s in src])
    rc = lib.ivosw_lstm_fwd_pair_probe(col(ops, 0), col(ops, 1), col(bufs, 0), col(bufs, 1), col(bufs, 2), col(bufs, 3),
                                       L.int_array([j[0] for j in jobs]), T, L.int_array([j[1] for j in jobs]), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("pair")
    for (N, keep_from, kept, seed), b in zip(jobs, bufs):
        o = _rec_read(b, N, T, keep_from)
        whh, gx, _, _, _ = _chain(N, T, seed)
        one = _lstm(dev, whh, gx, keep_from, R.FORM_MFMA, kept)
        _bit_equal([o.hs], [one.hs], f"pair job N={N}: hs")
        assert (o.gates is None) == (not kept)
        if kept:
            _bit_equal([o.gates, o.cs, o.hprev], [one.gates, one.cs, one.hprev], f"pair job N={N}")
        _hold(o, N, T, keep_from, R.FORM_MFMA, seed, what=f"pair job N={N}")


def test_lstm_fwd_ragged_slices_equal_quad1_on_each_slice(dev):
    """lstm_fwd_quad_ragged_kernel on lengths (1, 2, 9, 1) laid end to end: each slice is bit for bit lstm_fwd_quad_kernel<1> at N = 1 on
    that slice, and held by the chain yardstick."""
    lib = L.probe_lib()
    lens = R.RAGGED_LENGTHS
    rows = sum(lens)
    whh, gx, _, _, _ = _chain(1, rows, 2)
    (kw, pw), (kg, pg) = _op(whh, dev), _op(gx[0], dev)
    bh, ph = _out(rows, 256, dev)
    rc = lib.ivosw_lstm_fwd_ragged_probe(pw, pg, ph, L.int_array(lens), len(lens), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("ragged")
    hs = _kept(bh, rows, 0, "hs")
    r0 = 0
    for T in lens:
        sl = gx[:, r0:r0 + T]
        one = _lstm(dev, whh, sl, 1, 11)
        _bit_equal([hs[r0:r0 + T]], [one.hs[0]], f"slice at row {r0}, {T} frames")
        ref = R.lstm_fwd(whh, sl)[0]
        allowed = max(2 * R.rel_err(R.lstm_fwd(whh, sl, np.float32)[0], ref), 1e-6)
        assert R.rel_err(hs[r0:r0 + T][None], ref) <= allowed
        r0 += T


# ---------------------------------------------------------------- recurrence + decoder in one kernel
def _mega(dev, jobs, T):
    """jobs: (P, gx, keep_from, hs_from, kept) each -> [(Fwd, d1 kept rows, q)] of ONE brain_fwd_mega_kernel launch."""
    lib = L.probe_lib()
    ops = [(_op(R.arena(P)[:, None], dev), _op(gx.reshape(-1, 512), dev)) for P, gx, _, _, _ in jobs]
    bufs = [_rec_bufs(dev, gx.shape[0], T, kf, kept) for _, gx, kf, _, kept in jobs]
    outs = [(_out(gx.shape[0] * T, 128, dev), _out(gx.shape[0] * T, 1, dev)) for _, gx, _, _, _ in jobs]
    col = lambda src, i: _parr([_p(s[i]) for s in src])
    rc = lib.ivosw_fwd_mega_probe(len(jobs), col(ops, 0), col(ops, 1), col(bufs, 0), col(bufs, 1), col(bufs, 2), col(bufs, 3), col(outs, 0),
                                  col(outs, 1), L.int_array([j[1].shape[0] for j in jobs]), T, L.int_array([j[2] for j in jobs]),
                                  L.int_array([j[3] for j in jobs]), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("mega" if len(jobs) == 1 else "mega x2")
    res = []
    for (_, gx, kf, hf, kept), b, o in zip(jobs, bufs, outs):
        N = gx.shape[0]
        d1_from = kf if kept else N                          # without gates nothing is kept, d1 included
        res.append((_rec_read(b, N, T, kf, hf), _kept(o[0][0], N * T, d1_from * T, "d1"), _kept(o[1][0], N * T, 0, "q")[:, 0]))
    return res


def _mega_fixture(N, T, seed):
    P = _params(seed, False)
    return P, R.fwd_fixture(N, T, seed)[1]


def _mega_hold(dev, res, P, gx, keep_from, hs_from, kept, what):
    """The recurrence's outputs are lstm_fwd_mfma_kernel's bit for bit; d1 and q are within the decoder's bound of dec in float64 on the
    kernel's own hs (the MFMA form's, equal by the line before, for the samples whose hs the mega kernel does not store)."""
    o, d1, q = res
    N, T, _ = gx.shape
    one = _lstm(dev, P["lstm_cell.weight_hh"], gx, keep_from, R.FORM_MFMA, kept)
    _bit_equal([o.hs], [one.hs[hs_from:]], what + ": hs")
    if kept and keep_from < N:
        _bit_equal([o.gates, o.cs, o.hprev], [one.gates, one.cs, one.hprev], what)
    else:
        assert o.gates is None
    hs = np.concatenate([one.hs[:hs_from], o.hs]).reshape(N * T, 256)
    rd1, rq = R.dec(P, hs)
    b_d1, b_q = R.dec_bounds(P, hs)
    first = (keep_from if kept else N) * T
    r = (_ratio(d1, rd1[first:], b_d1[first:]) if first < N * T else 0.0, _ratio(q, rq, b_q))
    assert max(r) <= 1.0, f"{what}: d1, q are {r} x the decoder's bounds"
    return r


@pytest.mark.parametrize("N,T", [(N, T) for N in (4, 5) for T in R.MEGA_T])
def test_mega_recurrence_is_the_mfma_forms_and_its_decoder_is_within_the_decoders_bound(dev, N, T):
    """M = 2 T rows below, at and across the 64-row chunk; at N = 5 the last workgroup holds one sample (M = T).  (keep_from, hs_from) =
    (1, 2): hs only from sample 2, the kept buffers and d1 from sample 1; (0, 0): everything; (N, N): nothing but q."""
    P, gx = _mega_fixture(N, T, 0)
    worst = [0.0, 0.0]
    for keep_from, hs_from, kept in ((1, 2, True), (0, 0, True), (N, N, False)):
        res, = _mega(dev, [(P, gx, keep_from, hs_from, kept)], T)
        r = _mega_hold(dev, res, P, gx, keep_from, hs_from, kept, f"N={N} T={T} keep_from={keep_from} hs_from={hs_from}")
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"\nFIG mega N {N} T {T}: worst |.-ref64| / bound d1 {worst[0]:.3f}, q {worst[1]:.3f}")


def test_mega_two_jobs_with_different_arenas_each_equal_their_single_launch(dev):
    T = 33
    jobs = [_mega_fixture(5, T, 0) + (1, 0, True), _mega_fixture(4, T, 1) + (4, 2, False)]
    both = _mega(dev, jobs, T)
    for i, job in enumerate(jobs):
        one, = _mega(dev, [job], T)
        _bit_equal([both[i][0].hs, both[i][1], both[i][2]], [one[0].hs, one[1], one[2]], f"job {i}")
        _mega_hold(dev, both[i], *job, f"job {i}")


def test_mega_refuses_a_sequence_whose_rows_exceed_its_lds(dev):
    lib = L.probe_lib()
    N, T = 4, 74
    P, gx = _mega_fixture(N, T, 0)
    ops = (_op(R.arena(P)[:, None], dev), _op(gx.reshape(-1, 512), dev))
    bufs = _rec_bufs(dev, N, T, 0, True)
    outs = (_out(N * T, 128, dev), _out(N * T, 1, dev))
    one = lambda b: _parr([_p(b)])
    rc = lib.ivosw_fwd_mega_probe(1, one(ops[0]), one(ops[1]), one(bufs[0]), one(bufs[1]), one(bufs[2]), one(bufs[3]), one(outs[0]), one(outs[1]),
                                  L.int_array([N]), T, L.int_array([0]), L.int_array([0]), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _refused(lib, rc, "not covered", *[b[0] for b in bufs + outs])


# ---------------------------------------------------------------- reach and refusals
def test_every_forward_form_was_reached_by_a_case_of_its_own(dev):
    P, Pd = _params(0, True), _params(0, False)
    if "enc" not in REACHED:
        _enc(dev, [(P, R.enc_fixture(49, True), 49, 0)])
    if "enc x2" not in REACHED:
        test_enc_two_jobs_with_different_arenas_each_equal_their_single_launch(dev, True)
    if "dec" not in REACHED:
        _dec(dev, [(P, R.dec_fixture(49, True), 0)])
    if "dec x2" not in REACHED:
        test_dec_two_jobs_with_different_arenas_each_equal_their_single_launch(dev, True)
    for form, name in R.FORM_NAMES.items():
        if name not in REACHED:
            N = 5 if form == R.FORM_MFMA else 3
            _hold(_lstm(dev, *_chain(N, 2)[:2], 0, form), N, 2, 0, form)
    if "auto" not in REACHED:
        test_lstm_fwd_auto_is_the_products_choice_of_form(dev, 3)
    if "pair" not in REACHED:
        test_lstm_fwd_pair_jobs_each_equal_their_single_launch(dev)
    if "ragged" not in REACHED:
        test_lstm_fwd_ragged_slices_equal_quad1_on_each_slice(dev)
    if "mega" not in REACHED:
        _mega(dev, [_mega_fixture(5, 2, 0) + (1, 2, True)], 2)
    if "mega x2" not in REACHED:
        test_mega_two_jobs_with_different_arenas_each_equal_their_single_launch(dev)
    assert REACHED == {"enc", "enc x2", "dec", "dec x2", "auto", "pair", "ragged", "mega", "mega x2"} | set(R.FORM_NAMES.values())
    for name, (rg, rc, rh, ch) in sorted(WORST.items()):
        print(f"\nFIG lstm_fwd worst {name}: step gates {rg:.3f}, c {rc:.3f}, h {rh:.3f} of their allowances; chain {ch:.3f} of its allowance")


def test_forward_probes_refuse_what_the_kernels_do_not_take(dev):
    lib = L.probe_lib()
    st = L.stream_ptr(dev)
    ka, pa = _op(np.zeros((NPAD, 512), np.float32), dev)              # stands for every operand: zeros, large enough for any of them
    outs = [_out(8, 512, dev) for _ in range(6)]
    bufs = [b for b, _ in outs]
    po = [p for _, p in outs]
    one, i1 = lambda p: _parr([p]), lambda v: L.int_array([v])
    two, i2 = lambda p, q: _parr([p, q]), lambda a, b: L.int_array([a, b])

    enc = lambda prm=pa, x=pa, rows=1, rows0=1, keep=0, n=1, gx=po[0]: lib.ivosw_enc_fused_probe(
        n, one(prm), one(x), one(pa), i1(rows0), i1(rows), i1(keep), one(gx), one(po[1]), one(po[2]), st)
    _refused(lib, enc(prm=None), "null", *bufs)
    _refused(lib, enc(x=None), "null", *bufs)
    _refused(lib, enc(gx=None), "null", *bufs)
    _refused(lib, enc(rows=0, rows0=0), "not covered", *bufs)
    _refused(lib, enc(rows0=2), "not covered", *bufs)
    _refused(lib, enc(keep=2), "not covered", *bufs)
    _refused(lib, enc(n=3), "not covered", *bufs)
    _refused(lib, lib.ivosw_enc_fused_probe(1, None, one(pa), one(pa), i1(1), i1(1), i1(0), one(po[0]), one(po[1]), one(po[2]), st), "null", *bufs)

    dec = lambda prm=pa, hs=pa, rows=1, keep=0, n=1, q=po[1]: lib.ivosw_dec_fused_probe(n, one(prm), one(hs), i1(rows), i1(keep), one(po[0]), one(q), st)
    _refused(lib, dec(prm=None), "null", *bufs)
    _refused(lib, dec(hs=None), "null", *bufs)
    _refused(lib, dec(q=None), "null", *bufs)
    _refused(lib, dec(rows=0), "not covered", *bufs)
    _refused(lib, dec(keep=2), "not covered", *bufs)
    _refused(lib, dec(n=0), "not covered", *bufs)
    _refused(lib, dec(hs=L.torch_ptr(ka, 1)), "not covered", *bufs)

    ran = ctypes.c_int(-1)
    rec = lambda whh=pa, gx=pa, hs=po[0], gates=po[1], cs=po[2], hprev=po[3], N=1, T=1, kf=0, form=11: lib.ivosw_lstm_fwd_probe(
        whh, gx, hs, gates, cs, hprev, N, T, kf, form, ctypes.byref(ran), st)
    _refused(lib, rec(whh=None), "null", *bufs)
    _refused(lib, rec(gx=None), "null", *bufs)
    _refused(lib, rec(hs=None), "null", *bufs)
    _refused(lib, rec(cs=None), "not covered", *bufs)                  # gates without cs
    _refused(lib, rec(N=0), "not covered", *bufs)
    _refused(lib, rec(T=0), "not covered", *bufs)
    _refused(lib, rec(kf=2), "not covered", *bufs)
    _refused(lib, rec(N=3, form=R.FORM_MFMA), "not covered", *bufs)     # six rows: the product never sends the MFMA form fewer than eight
    for form in (3, 8, 10, 13, 21, -1):
        _refused(lib, rec(form=form), "not covered", *bufs)
    assert ran.value == -1

    pair = lambda whh=pa, hs=po[0], N=4, T=1, kf=0: lib.ivosw_lstm_fwd_pair_probe(two(pa, whh), two(pa, pa), two(po[4], hs), two(po[1], None),
                                                                                 two(po[2], None), two(po[3], None), i2(4, N), T, i2(kf, 0), st)
    _refused(lib, pair(whh=None), "null", *bufs)
    _refused(lib, pair(hs=None), "null", *bufs)
    _refused(lib, pair(N=3), "not covered", *bufs)
    _refused(lib, pair(N=0), "not covered", *bufs)
    _refused(lib, pair(T=0), "not covered", *bufs)
    _refused(lib, pair(kf=5), "not covered", *bufs)

    rag = lambda whh=pa, hs=po[0], lens=(1, 2), n=2: lib.ivosw_lstm_fwd_ragged_probe(whh, pa, hs, L.int_array(lens), n, st)
    _refused(lib, rag(whh=None), "null", *bufs)
    _refused(lib, rag(hs=None), "null", *bufs)
    _refused(lib, lib.ivosw_lstm_fwd_ragged_probe(pa, pa, po[0], None, 2, st), "null", *bufs)
    assert rag(lens=(1, 0)) != 0 and rag(n=0) != 0 and _untouched(*bufs)          # a length or a count below 1: the entry point's own refusals

    mega = lambda prm=pa, q=po[5], N=4, T=1, kf=0, hf=0, n=1, cs=po[2]: lib.ivosw_fwd_mega_probe(
        n, one(prm), one(pa), one(po[0]), one(po[1]), one(cs), one(po[3]), one(po[4]), one(q), i1(N), T, i1(kf), i1(hf), st)
    _refused(lib, mega(prm=None), "null", *bufs)
    _refused(lib, mega(q=None), "null", *bufs)
    _refused(lib, mega(cs=None), "not covered", *bufs)
    _refused(lib, mega(N=3), "not covered", *bufs)
    _refused(lib, mega(N=0), "not covered", *bufs)
    _refused(lib, mega(T=0), "not covered", *bufs)
    _refused(lib, mega(T=74), "not covered", *bufs)
    _refused(lib, mega(hf=5), "not covered", *bufs)
    _refused(lib, mega(n=3), "not covered", *bufs)
    torch.cuda.synchronize(dev)

