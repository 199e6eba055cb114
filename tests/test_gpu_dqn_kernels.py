"""The backward kernels of the DQN step - bwd_tail_kernel's three units (wgrad_tile, dgrad_tile, csum_unit; csrc/brain_bwd.h), the step's two
grouped launches of it with the slab reduction, head_fused_kernel<false|true> (csrc/dqn_head.h), lstm_bwd_quad_kernel<1> and
lstm_bwd_kernel<1|2|4> (csrc/lstm_bwd.h) - each ALONE through its probe entry (include/ivosw_probe.h, libivosw_probe.so) on tensors this file
makes, against the float64 restatements of tests/dqn_ref.py (pinned to the oracle on the CPU by tests/test_dqn_ref.py).  The rules are
those of tests/test_gpu_layer_kernels.py:

  reach   every unit of bwd_tail_kernel, the grouped form, both head instantiations and the four recurrence forms ran in a case of their own
  exact   small-integer operands whose sums no fp32 order can change: the output equals float64, zero tolerance
  dense   random operands: |y - ref64| <= (K + 2) 2^-23 sum_k |a_k| |b_k| per element, the worst case of an fp32 sum of K products in any
          order (dqn_ref.sum_bound); the recurrence, which evaluates tanh on the device, against the project's own yardstick
          max(2 x the fp32 numpy restatement's error, 1e-6) of the tensor's largest element
  guards  every output sits between guard rows of a NaN pattern that must stay; every row-indexed operand is followed by NaN guard rows, so
          a read past K or `rows` shows in the output (the kernels clamp tail reads to the last live row)
  refuse  what a kernel does not take is refused and nothing is written

Measured figures: LAB_NOTES.md, "DQN backward kernels alone"."""
import ctypes

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from tests import dqn_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4               # guard rows
REACHED = set()
NAN32 = np.int32(R.NAN_BITS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _op(a, dev, ld=None, col0=0):
    """Operand a [rows, cols] (or 1-D) on the device inside a [rows + GUARD, ld] buffer of the NaN pattern at column col0; -> (buffer, pointer)."""
    a = np.ascontiguousarray(a, np.float32)
    a2 = a.reshape(a.shape[0], -1)
    ld = ld or a2.shape[1]
    host = np.full((a2.shape[0] + GUARD, ld), NAN32, np.int32)
    host[:a2.shape[0], col0:col0 + a2.shape[1]] = a2.view(np.int32)
    buf = torch.from_numpy(host).to(dev)
    return buf, L.torch_ptr(buf, col0)


def _out(rows, cols, dev):
    """Output of rows x cols floats between GUARD guard rows of the NaN pattern; -> (buffer, pointer of row 0)."""
    buf = torch.full((rows + 2 * GUARD, cols), R.NAN_BITS, dtype=torch.int32, device=dev)
    return buf, L.torch_ptr(buf, GUARD * cols)


def _read(buf, rows):
    """-> (the rows as float32, True if everything around them still holds the pattern)."""
    h = buf.cpu().numpy()
    clean = bool((h[:GUARD] == NAN32).all() and (h[GUARD + rows:] == NAN32).all())
    return h[GUARD:GUARD + rows].view(np.float32), clean


def _untouched(*bufs):
    return all(bool((b == R.NAN_BITS).all()) for b in bufs)


def _ok(lib, rc):
    assert rc == 0, lib.ivosw_last_error().decode()


def _same(got, want64, what):
    """got (float32) equals the float64 reference element for element."""
    bad = got.astype(np.float64) != want64
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} elements differ from float64; first at {i}: got {got[i]!r}, want {want64[i]!r}")


def _ratio(got, want64, bound):
    """worst |got - ref64| / bound over the elements (0 / 0 counts as 0: an exact zero where nothing can err)."""
    err = np.abs(got.astype(np.float64) - want64)
    assert np.isfinite(got).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ---------------------------------------------------------------- wgrad
def _wgrad(dev, M, N, lda, K, nslab, kind, has2, exact):
    lib = L.probe_lib()
    A, A2, B = R.wgrad_fixture(M, N, K, has2, exact)
    col0 = R.WG_COL0 if lda > M else 0
    (ka, pa), (kb, pb) = _op(A, dev, lda, col0), _op(B, dev)
    ka2, pa2 = _op(A2, dev, lda, col0) if has2 else (None, None)
    cap = nslab if nslab else 64
    buf, pc = _out(cap + 1, M * N, dev)              # one slab more than any count that may run: it has to stay NaN
    used = ctypes.c_int(-1)
    rc = lib.ivosw_bwd_wgrad_probe(pa, pa2, pb, pc, lda, N, M, N, K, nslab, kind, ctypes.byref(used), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("wgrad")
    ns = used.value
    assert 1 <= ns <= cap and (nslab == 0 or ns == nslab)
    got, clean = _read(buf, ns)
    assert clean, "a slab past nslab or a guard row was written"
    got = got.reshape(ns, M, N)
    assert np.isfinite(got).all(), "a slab element was not written, or a guard row of an operand reached it"
    return got, (A, A2, B), ns


WG_CASES = [(K, 1, 0) for K in R.WG_K1] + [(K, ns, 0) for K, ns in R.WG_SPLITS] + [(K, 0, kind) for K, kind in R.WG_AUTO]


@pytest.mark.parametrize("M,N,lda", R.WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_exact_fixture_is_bit_equal_to_fp64_slab_by_slab(dev, M, N, lda):
    """Operands in {-2 .. 2}: every slab of C equals float64, A2 present and NULL, at every K of the table (each residue of the 16-row step,
    each unroll phase ending the loop, each wave's 4-row group the last live one), K = 97 in 2, 3 and 7 slabs (empty trailing slabs are
    zeros) and the product's own slab choice at K = 3225 (dW_ih) and K = 6450 (dW_hh)."""
    for K, nslab, kind in WG_CASES:
        for has2 in (False, True):
            got, (A, A2, B), ns = _wgrad(dev, M, N, lda, K, nslab, kind, has2, True)
            _same(got, R.wgrad_slabs(A, A2, B, ns), f"K={K} nslab={ns} A2={has2}")
            for z, (lo, hi) in enumerate(R.slab_rows(K, ns, 16)):
                if lo == hi:
                    assert not got[z].any(), f"K={K}: empty slab {z} is not zero"
    assert R.slab_rows(97, 7, 16)[-1] == (96, 97) and R.slab_rows(33, 7, 16)[3] == (33, 33)


def test_wgrad_empty_trailing_slabs_are_exact_zeros(dev):
    """K = 33 in 7 slabs of 16 rows: slabs 3 .. 6 have no rows at all."""
    got, (A, A2, B), ns = _wgrad(dev, 128, 128, 128, 33, 7, 0, True, True)
    _same(got, R.wgrad_slabs(A, A2, B, 7), "K=33 nslab=7")
    assert not got[3:].any() and got[:3].any()


@pytest.mark.parametrize("M,N,lda", R.WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_dense_fixture_is_within_its_derived_bound_of_fp64(dev, M, N, lda):
    """|C - ref64| <= (Kslab + 2) 2^-23 sum_k |a_k| |b_k| per element and slab."""
    worst = 0.0
    for K, nslab, kind in WG_CASES:
        for has2 in (False, True):
            got, (A, A2, B), ns = _wgrad(dev, M, N, lda, K, nslab, kind, has2, False)
            rows = R.slab_rows(K, ns, 16)
            bound = np.stack([R.sum_bound(hi - lo, m) for (lo, hi), m in zip(rows, R.wgrad_mag(A, A2, B, ns))])
            r = _ratio(got, R.wgrad_slabs(A, A2, B, ns), bound)
            worst = max(worst, r)
            assert r <= 1.0, f"K={K} nslab={ns} A2={has2}: an element is {r:.2f} x its bound"
    print(f"\nFIG wgrad {M}x{N} lda {lda}: worst |C-ref64| / bound {worst:.3f}")


# ---------------------------------------------------------------- dgrad
def _dgrad(dev, rows, exact):
    lib = L.probe_lib()
    fx = R.dgrad_fixture(rows, exact)
    keep = [_op(t, dev) for t in fx]
    (bde, pde), (bda, pda) = _out(rows, 128, dev), _out(rows, 128, dev)
    rc = lib.ivosw_bwd_dgrad_probe(*[p for _, p in keep], pde, pda, rows, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("dgrad")
    (de, c1), (da1, c2) = _read(bde, rows), _read(bda, rows)
    assert c1 and c2, "rows at `rows` and beyond were written"
    assert np.isfinite(de).all() and np.isfinite(da1).all()
    return de, da1, fx


@pytest.mark.parametrize("rows", R.DG_ROWS)
def test_dgrad_exact_fixture_is_bit_equal_to_fp64(dev, rows):
    de, da1, fx = _dgrad(dev, rows, True)
    rde, rda1 = R.dgrad(*fx)
    _same(de, rde, "de")
    _same(da1, rda1, "da1")
    assert not da1[~(fx[4] > 0)].any()


@pytest.mark.parametrize("rows", R.DG_ROWS)
def test_dgrad_dense_fixture_is_within_its_derived_bound_and_masks_as_fp64(dev, rows):
    de, da1, fx = _dgrad(dev, rows, False)
    rde, rda1 = R.dgrad(*fx)
    bde, bda1 = R.dgrad_bounds(*fx[:4])
    r1, r2 = _ratio(de, rde, bde), _ratio(da1, rda1, bda1)
    print(f"\nFIG dgrad rows {rows}: worst |de-ref64| / bound {r1:.3f}, |da1-ref64| / bound {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0
    assert np.array_equal(da1 == 0, rda1 == 0), "the a1 > 0 mask: zero pattern differs from the reference's"
    assert np.array_equal(da1 == 0, ~(fx[4] > 0))          # +0, -0 and negatives mask, the smallest subnormal does not


# ---------------------------------------------------------------- csum
def _csum(dev, M, N, ld, nsplit, with_x, exact):
    lib = L.probe_lib()
    A, x = R.csum_fixture(M, N, with_x, exact)
    (ka, pa) = _op(A, dev, ld)
    kx, px = _op(x, dev) if with_x else (None, None)
    bo, po = _out(nsplit, N, dev)
    bw, pw = _out(nsplit, 2 * N, dev)
    rc = lib.ivosw_bwd_csum_probe(pa, px, po, pw if with_x else None, M, N, ld, nsplit, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("csum")
    (out, c1), (outw, c2) = _read(bo, nsplit), _read(bw, nsplit)
    assert c1 and c2, "a guard row was written"
    if not with_x:
        assert _untouched(bw), "outw written without x"
    assert np.isfinite(out).all() and (not with_x or np.isfinite(outw).all())
    return out, outw.reshape(nsplit, N, 2), A, x


CS_CASES = [(M, 128, ns) for M in R.CS_M for ns in R.CS_SPLITS] + [(65, 100, 8), (9, 100, 1)]


@pytest.mark.parametrize("with_x", (False, True), ids=("plain", "x"))
def test_csum_exact_fixture_is_bit_equal_to_fp64(dev, with_x):
    """Every M of the table (the 64-row loop, the 8-row tail, fewer rows than row groups) in 1 and 8 splits, N = 128 and N = 100 in a row of
    128 whose columns past N hold NaNs; splits without rows are zeros."""
    for M, N, ns in CS_CASES:
        out, outw, A, x = _csum(dev, M, N, 128, ns, with_x, True)
        ro, rw = R.csum_slabs(A, x, ns)
        _same(out, ro, f"out M={M} N={N} nsplit={ns}")
        if with_x:
            _same(outw, rw, f"outw M={M} N={N} nsplit={ns}")
        for z, (lo, hi) in enumerate(R.slab_rows(M, ns, 8)):
            if lo == hi:
                assert not out[z].any() and not (with_x and outw[z].any()), f"M={M}: empty split {z} is not zero"


def test_csum_dense_fixture_is_within_its_derived_bound_of_fp64(dev):
    worst = 0.0
    for M, N, ns in CS_CASES:
        out, outw, A, x = _csum(dev, M, N, 128, ns, True, False)
        ro, rw = R.csum_slabs(A, x, ns)
        a = np.abs(A.astype(np.float64))
        for z, (lo, hi) in enumerate(R.slab_rows(M, ns, 8)):
            r = max(_ratio(out[z], ro[z], R.sum_bound(hi - lo, a[lo:hi].sum(0))),
                    _ratio(outw[z], rw[z], R.sum_bound(hi - lo, a[lo:hi].T @ np.abs(x[lo:hi].astype(np.float64)))))
            worst = max(worst, r)
            assert r <= 1.0, f"M={M} N={N} nsplit={ns} split {z}: {r:.2f} x the bound"
    print(f"\nFIG csum: worst |sum-ref64| / bound {worst:.3f}")


# ---------------------------------------------------------------- the step's two launches + reduction
@pytest.mark.parametrize("B,T", R.GROUP_BT)
def test_group_exact_fixture_every_gradient_is_bit_equal_to_fp64(dev, B, T):
    """dgrad tiles + dW_hh + dW_ih + dW3, then dW2 + four column sums, then the slab reduction, as the step builds them (plan_bwd_tail): integer
    operands, so de, da1 and the nine gradient tensors these launches produce equal float64 - one dropped or doubled row anywhere shows.
    decoder_fc2.bias is the head kernel's: its slot, like everything around the arena, keeps the pattern."""
    lib = L.probe_lib()
    fx = R.group_fixture(B, T)
    rows = B * T
    order = ("dG", "hprev", "e", "a1", "dd1c", "hcc", "w4term", "state", "wih", "w2")
    keep = [_op(fx[k].reshape(-1, fx[k].shape[-1]), dev) for k in order]
    (bde, pde), (bda, pda) = _out(rows, 128, dev), _out(rows, 128, dev)
    bg = torch.full((R.NPARAMS + 2 * 1024,), R.NAN_BITS, dtype=torch.int32, device=dev)
    ws = torch.full((L.BWD_GROUP_WS_FLOATS + 1024,), R.NAN_BITS, dtype=torch.int32, device=dev)
    rc = lib.ivosw_bwd_group_probe(*[p for _, p in keep], pde, pda, L.torch_ptr(bg, 1024), L.dptr(ws), B, T, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("group")
    rde, rda1, G = R.tail_grads(**fx)
    (de, c1), (da1, c2) = _read(bde, rows), _read(bda, rows)
    assert c1 and c2 and bool((ws[L.BWD_GROUP_WS_FLOATS:] == R.NAN_BITS).all()), "a guard was written"
    _same(de, rde, "de")
    _same(da1, rda1, "da1")
    g = bg.cpu().numpy()
    assert (g[:1024] == NAN32).all() and (g[1024 + R.NPARAMS:] == NAN32).all(), "written outside the arena"
    arena = g[1024:1024 + R.NPARAMS]
    for name, off, shape in R.ARENA:
        n = int(np.prod(shape))
        if name == "decoder_fc2.bias":
            assert arena[off] == NAN32
            continue
        _same(arena[off:off + n].view(np.float32).reshape(shape), G[name], name)


# ---------------------------------------------------------------- head
def _head(dev, fx, B, T, kind, per, gamma=R.HEAD_GAMMA, delta=R.HEAD_DELTA):
    lib = L.probe_lib()
    prm = np.concatenate([np.full(16, np.nan, np.float32), fx["W3"].ravel(), fx["w4"]])
    kp, pp = _op(prm[:, None], dev)
    ins = [_op(fx[k].reshape(B, -1), dev) for k in ("q_np", "q_nt", "q_s")]
    act = torch.from_numpy(fx["action"]).to(dev)
    rs, rd, d1, hs, wt = (_op(fx[k].reshape(B, -1), dev) for k in ("r_step", "r_done", "d1", "hs", "weights"))
    outs = {k: _out(B, c, dev) for k, c in (("dq", 1), ("dd1c", 128), ("w4term", 128), ("hcc", 256), ("dhc", 256), ("td", 1))}
    outs["loss"], outs["db4"] = _out(1, 1, dev), _out(1, 1, dev)
    o = lambda k: outs[k][1]
    rc = lib.ivosw_head_fused_probe(pp, 16, 16 + 128 * 256, ins[0][1], ins[1][1], ins[2][1], L.dptr(act), rs[1], rd[1], B, T, gamma, kind, delta,
                                    d1[1], hs[1], o("dq"), o("dd1c"), o("w4term"), o("hcc"), o("dhc"), o("loss"), o("db4"), per,
                                    wt[1] if per else None, o("td") if per else None, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("head<true>" if per else "head<false>")
    got = {}
    for k, (buf, _) in outs.items():
        if k == "td" and not per:
            assert _untouched(buf), "td written by the unweighted kernel"
            continue
        n = 1 if k in ("loss", "db4") else B
        got[k], clean = _read(buf, n)
        assert clean, f"{k}: a guard row was written"
        assert np.isfinite(got[k]).all(), k
    return got


@pytest.mark.parametrize("per", (0, 1), ids=("plain", "per"))
def test_head_argmax_is_the_first_maximum(dev, per):
    """With q_nt[b][t] = t, gamma = 1, zero rewards and zero Q(s, a) the kernel's frame choice comes out as a number: td = am exactly
    (weighted kernel), dq = -(2 / B) am (both).  Ties at the first and last frame, an all-equal row, 64-lane groups of every length."""
    for B, T in ((3, 1), (5, 63), (5, 64), (257, 65)):
        fx = R.head_fixture(B, T)
        fx["q_nt"] = np.tile(np.arange(T, dtype=np.float32), (B, 1))
        fx["q_s"] = np.zeros((B, T), np.float32)
        fx["r_step"] = fx["r_done"] = np.zeros(B, np.float32)
        fx["weights"] = np.ones(B, np.float32)
        got = _head(dev, fx, B, T, R.LOSS_MSE, per, gamma=1.0)
        am = R.first_argmax(fx["q_np"])
        assert am[0] == 0 and (B < 3 or T < 3 or am[2] == 14 % T)
        if per:
            assert np.array_equal(got["td"][:, 0], am.astype(np.float32)), "td"
        assert np.array_equal(np.rint(-got["dq"][:, 0].astype(np.float64) * B / 2).astype(np.int64), am), "dq"


@pytest.mark.parametrize("B,T,kind,per", R.head_cases())
def test_head_against_fp32_restatement_and_fp64(dev, B, T, kind, per):
    """dq and td within 2 ulp of the fp32 restatement; w4term, dd1c, hcc exactly what fp32 gives from the kernel's own dq, with the
    reference's zero patterns; dhc within the K = 128 bound of float64 from that dq, zero exactly where h is not positive; loss and db4
    within the K = B bound of float64 (dqn_ref.head_bounds)."""
    fx = R.head_fixture(B, T)
    got = _head(dev, fx, B, T, kind, per)
    args = (fx["W3"], fx["w4"], fx["q_np"], fx["q_nt"], fx["q_s"], fx["action"], fx["r_step"], fx["r_done"], R.HEAD_GAMMA, kind, R.HEAD_DELTA,
            fx["d1"], fx["hs"], fx["weights"] if per else None)
    r32, r64 = R.head(*args, dtype=np.float32), R.head(*args, dtype=np.float64)
    assert set(fx["action"].tolist()) >= ({0, T - 1} if B > 1 else {0})
    dq = got["dq"][:, 0]
    u = float(R.ulps32(dq, r32["dq_own"]).max())
    ut = float(R.ulps32(got["td"][:, 0], r32["td"]).max()) if per else 0.0
    assert u <= 2 and ut <= 2, f"dq {u} ulp, td {ut} ulp from the fp32 restatement"
    own32, own64 = R.head(*args, dtype=np.float32, dq=dq), R.head(*args, dtype=np.float64, dq=dq)
    for k in ("w4term", "dd1c", "hcc"):
        assert np.array_equal(got[k], own32[k]), k
    for k in ("dd1c", "hcc"):            # (w4term = dq d1 underflows in fp32 where d1 is the subnormal: it has no mask of its own)
        assert np.array_equal(got[k] == 0, own64[k] == 0), f"{k}: zero pattern"
    assert np.array_equal(got["dhc"] == 0, own64["dhc"] == 0), "dhc: zero pattern"
    rd = _ratio(got["dhc"], own64["dhc"], R.sum_bound(128, own64["mag_dhc"]))
    bl, bb = R.head_bounds(r64, B)
    rl, rb = abs(float(got["loss"][0, 0]) - r64["loss"]) / bl, abs(float(got["db4"][0, 0]) - r64["db4"]) / bb
    print(f"\nFIG head B {B} T {T} kind {kind} per {per}: dq {u:.2f} ulp, td {ut:.2f} ulp, dhc {rd:.3f}, loss {rl:.3f}, db4 {rb:.3f} of their bounds")
    assert rd <= 1.0 and rl <= 1.0 and rb <= 1.0


# ---------------------------------------------------------------- BPTT recurrence
def _lstm(dev, fx, N, T, form):
    lib = L.probe_lib()
    keep = [_op(fx[k].reshape(-1, fx[k].shape[-1]), dev) for k in ("whh", "gates", "cs", "dhc")]
    act = torch.from_numpy(fx["action"]).to(dev)
    buf, pg = _out(2 * N * T, 512, dev)
    rc = lib.ivosw_lstm_bwd_probe(keep[0][1], keep[1][1], keep[2][1], keep[3][1], L.dptr(act), pg, N, T, form, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    _ok(lib, rc)
    REACHED.add("lstm_quad<1>" if form == 0 else f"lstm<{form}>")
    dG, clean = _read(buf, 2 * N * T)
    assert clean, "a guard row was written"
    assert np.isfinite(dG).all(), "a frame was neither computed nor zero-filled"
    return dG.reshape(2, N, T, 512)


@pytest.mark.parametrize("N,T", [(N, T) for N in (1, 3, 130) for T in R.LSTM_T])
def test_lstm_bwd_forms_against_fp64_with_the_fp32_restatements_yardstick(dev, N, T):
    """Every form that takes this N: dG is exactly zero at the frames past the loss frame (both directions), and on the live frames within
    max(2 x the fp32 numpy restatement's error, 1e-6) of float64, relative to dG's largest element; the forms agree within the same figure."""
    fx = R.lstm_fixture(N, T)
    ref = R.bptt(**fx)
    e32 = R.rel_err(R.bptt(**fx, dtype=np.float32), ref)
    allowed = max(2 * e32, 1e-6)
    live = R.live_frames(fx["action"], N, T)
    first = None
    for form in [f for f, ns in R.LSTM_N.items() if N in ns]:
        dG = _lstm(dev, fx, N, T, form)
        assert not dG[~live].any(), f"form {form}: a frame past the loss frame is not zero"
        err = R.rel_err(dG, ref)
        print(f"\nFIG lstm_bwd N {N} T {T} form {form}: fp32 numpy {e32:.3e}, kernel {err:.3e}, allowed {allowed:.3e}")
        assert err <= allowed, f"form {form}"
        if first is None:
            first = dG
        else:
            d = float(np.abs(dG.astype(np.float64) - first).max() / np.abs(ref).max())
            assert d <= allowed, f"form {form} differs from the first form by {d:.3e}"


# ---------------------------------------------------------------- reach and refusals
def test_every_kernel_was_reached_by_a_case_of_its_own(dev):
    if "wgrad" not in REACHED:
        _wgrad(dev, 128, 128, 128, 17, 1, 0, True, True)
    if "dgrad" not in REACHED:
        _dgrad(dev, 17, True)
    if "csum" not in REACHED:
        _csum(dev, 9, 128, 128, 1, True, True)
    if "group" not in REACHED:
        test_group_exact_fixture_every_gradient_is_bit_equal_to_fp64(dev, 4, 3)
    for per in (0, 1):
        if ("head<true>" if per else "head<false>") not in REACHED:
            _head(dev, R.head_fixture(2, 3), 2, 3, R.LOSS_MSE, per)
    for form in (0, 1, 2, 4):
        if ("lstm_quad<1>" if form == 0 else f"lstm<{form}>") not in REACHED:
            _lstm(dev, R.lstm_fixture(3, 2), 3, 2, form)
    assert REACHED == {"wgrad", "dgrad", "csum", "group", "head<false>", "head<true>", "lstm_quad<1>", "lstm<1>", "lstm<2>", "lstm<4>"}


def _refused(lib, rc, word, *bufs):
    err = lib.ivosw_last_error().decode()
    assert rc != 0 and word in err, (rc, err)
    assert _untouched(*bufs), "a refused call wrote"


def test_probes_refuse_what_the_kernels_do_not_take(dev):
    lib = L.probe_lib()
    st = L.stream_ptr(dev)
    A, A2, B = R.wgrad_fixture(128, 128, 16, True, True)
    (ka, pa), (ka2, pa2), (kb, pb) = _op(A, dev), _op(A2, dev), _op(B, dev)
    bc, pc = _out(2, 128 * 128, dev)
    used = ctypes.c_int(-1)
    for M, N, K in ((96, 128, 16), (128, 64, 16), (128, 128, 0)):
        _refused(lib, lib.ivosw_bwd_wgrad_probe(pa, pa2, pb, pc, 128, 128, M, N, K, 1, 0, ctypes.byref(used), st), "not covered", bc)
    _refused(lib, lib.ivosw_bwd_wgrad_probe(pa, pa2, pb, pc, 128, 128, 128, 128, 16, 0, 3, ctypes.byref(used), st), "not covered", bc)
    _refused(lib, lib.ivosw_bwd_wgrad_probe(None, pa2, pb, pc, 128, 128, 128, 128, 16, 1, 0, ctypes.byref(used), st), "null", bc)
    _refused(lib, lib.ivosw_bwd_wgrad_probe(pa, pa2, None, pc, 128, 128, 128, 128, 16, 1, 0, ctypes.byref(used), st), "null", bc)
    assert used.value == -1

    fx = R.dgrad_fixture(16, True)
    ops = [_op(t, dev) for t in fx]
    (bde, pde), (bda, pda) = _out(16, 128, dev), _out(16, 128, dev)
    ptrs = [p for _, p in ops]
    _refused(lib, lib.ivosw_bwd_dgrad_probe(*ptrs, pde, pda, 0, st), "not covered", bde, bda)
    _refused(lib, lib.ivosw_bwd_dgrad_probe(*ptrs[:4], None, pde, pda, 16, st), "null", bde, bda)

    (bo, po), (bw, pw) = _out(1, 128, dev), _out(1, 256, dev)
    _refused(lib, lib.ivosw_bwd_csum_probe(None, None, po, None, 16, 128, 128, 1, st), "null", bo, bw)
    _refused(lib, lib.ivosw_bwd_csum_probe(ptrs[4], None, po, pw, 16, 128, 128, 1, st), "go together", bo, bw)
    _refused(lib, lib.ivosw_bwd_csum_probe(ptrs[4], None, po, None, 0, 128, 128, 1, st), "not covered", bo, bw)

    bg = torch.full((R.NPARAMS,), R.NAN_BITS, dtype=torch.int32, device=dev)
    args = [pa] * 9 + [None, pde, pda, L.dptr(bg), pc]
    _refused(lib, lib.ivosw_bwd_group_probe(*args, 1, 1, st), "null", bde, bda, bg, bc)
    args[9] = pa
    _refused(lib, lib.ivosw_bwd_group_probe(*args, 0, 3, st), "not covered", bde, bda, bg, bc)

    outs = [_out(1, 256, dev) for _ in range(8)]
    op = [p for _, p in outs]
    act = torch.zeros(1, dtype=torch.int64, device=dev)
    head = lambda q, per, w, B: lib.ivosw_head_fused_probe(pa, 0, 0, q, pa, pa, L.dptr(act), pa, pa, B, 1, 0.5, 0, 1.0, pa, pa, op[0], op[1], op[2],
                                                           op[3], op[4], op[5], op[6], per, w, op[7], st)
    _refused(lib, head(None, 0, None, 1), "null", *[b for b, _ in outs])
    _refused(lib, head(pa, 1, None, 1), "null", *[b for b, _ in outs])
    _refused(lib, head(pa, 0, None, 0), "not covered", *[b for b, _ in outs])

    bG, pG = _out(2, 512, dev)
    _refused(lib, lib.ivosw_lstm_bwd_probe(pa, pa, pa, None, L.dptr(act), pG, 1, 1, 0, st), "null", bG)
    _refused(lib, lib.ivosw_lstm_bwd_probe(pa, pa, pa, pa, L.dptr(act), pG, 1, 1, 3, st), "not covered", bG)
    _refused(lib, lib.ivosw_lstm_bwd_probe(pa, pa, pa, pa, L.dptr(act), pG, 0, 1, 0, st), "not covered", bG)
    torch.cuda.synchronize(dev)
