"""Float64 restatements, in plain numpy, of what the DQN step's backward kernels compute (csrc/brain_bwd.h: wgrad_tile, dgrad_tile, csum_unit;
csrc/dqn_head.h: head_fused_kernel; csrc/lstm_bwd.h: lstm_bwd_quad_kernel, lstm_bwd_kernel), one function per operation, and the fixtures
of tests/test_gpu_dqn_kernels.py.  tests/test_dqn_ref.py pins the functions, composed in the step's order, to
oracle.brain_oracle.dqn_loss_and_grads(..., dtype=np.float64) and asserts every fixture's preconditions - no GPU is needed for either.
The second half of the file does the same for the Brain forward kernels (tests/test_gpu_dqn_fwd_kernels.py): enc, dec, lstm_step, lstm_fwd,
their bounds and fixtures, pinned to oracle.brain_oracle.brain_forward(..., np.float64, keep=True).

Every function takes a dtype: float64 is the reference, float32 the "same restatement in fp32" that the yardsticks of the GPU tests name."""
import numpy as np

H = 128
NAN_BITS = 0x7FC0A5A5                     # the guard pattern (a quiet NaN) as int32
U23 = 2.0 ** -23
SUBNORMAL = np.float32(1.401298464324817e-45)       # the smallest positive fp32 subnormal
LOSS_MSE, LOSS_HUBER = 0, 1


# ---------------------------------------------------------------- slabs
def slab_rows(K, nslab, step):
    """Row ranges of the K-slabs as wgrad_tile (step 16) and csum_unit (step 8) cut them: ceil(K / nslab) rounded up to the step."""
    per = -(-(-(-K // nslab)) // step) * step
    return [(min(K, z * per), min(K, (z + 1) * per)) for z in range(nslab)]


# ---------------------------------------------------------------- weight gradient  C = (A + A2)^T B
def wgrad(A, A2, B, dtype=np.float64):
    """A, A2 [K,M], B [K,N] -> C [M,N]."""
    a = A.astype(dtype) + (A2.astype(dtype) if A2 is not None else dtype(0))
    return a.T @ B.astype(dtype)


def wgrad_slabs(A, A2, B, nslab, dtype=np.float64):
    """-> [nslab,M,N], slab z over its own rows (an empty slab is zeros)."""
    return np.stack([wgrad(A[lo:hi], None if A2 is None else A2[lo:hi], B[lo:hi], dtype) for lo, hi in slab_rows(A.shape[0], nslab, 16)])


def wgrad_mag(A, A2, B, nslab):
    """sum_k |a_k| |b_k| per slab and element: what the fp32 sum's bound scales with, and what the exact fixtures keep below 2^24."""
    a = np.abs(A.astype(np.float64) + (A2.astype(np.float64) if A2 is not None else 0.0))
    b = np.abs(B.astype(np.float64))
    return np.stack([a[lo:hi].T @ b[lo:hi] for lo, hi in slab_rows(A.shape[0], nslab, 16)])


def sum_bound(K, mag):
    """|fp32 sum of K products in any order - exact| <= (K + 2) 2^-23 sum |a_k| |b_k| (tests/layer_ref.py's rule: K - 1 additions and the
    products' roundings at half an ulp each, rounded up generously; the + 2 also covers A + A2's rounding)."""
    return (K + 2) * U23 * mag


# ---------------------------------------------------------------- dgrad chain
def dgrad(dG, dG2, wih, w2, a1, dtype=np.float64):
    """de = (dG + dG2) W_ih, da1 = (de W2) * (a1 > 0).  dG, dG2 [rows,512], wih [512,128], w2 [128,128], a1 [rows,128]."""
    de = (dG.astype(dtype) + dG2.astype(dtype)) @ wih.astype(dtype)
    da1 = (de @ w2.astype(dtype)) * (a1 > 0)
    return de, da1


def dgrad_bounds(dG, dG2, wih, w2):
    """(bound of de, bound of da1) per element.  de: K = 512.  da1, two stages: the kernel multiplies ITS de (within bde of the reference's), so
    K = 128 on (|de| + bde) |w2| plus bde carried through |w2|."""
    dgx = np.abs(dG.astype(np.float64) + dG2.astype(np.float64))
    bde = sum_bound(512, dgx @ np.abs(wih.astype(np.float64)))
    de = np.abs((dG.astype(np.float64) + dG2.astype(np.float64)) @ wih.astype(np.float64))
    aw2 = np.abs(w2.astype(np.float64))
    return bde, sum_bound(128, (de + bde) @ aw2) + bde @ aw2


# ---------------------------------------------------------------- column sums
def csum(A, x=None, dtype=np.float64):
    """A [M,N] -> out [N]; with x [M,2] also outw [N,2] = A^T x."""
    a = A.astype(dtype)
    return a.sum(0), (None if x is None else a.T @ x.astype(dtype))


def csum_slabs(A, x, nsplit, dtype=np.float64):
    outs, outws = [], []
    for lo, hi in slab_rows(A.shape[0], nsplit, 8):
        o, ow = csum(A[lo:hi], None if x is None else x[lo:hi], dtype)
        outs.append(o)
        outws.append(ow)
    return np.stack(outs), (None if x is None else np.stack(outws))


# ---------------------------------------------------------------- the head
def first_argmax(q):
    """First maximum per row (torch CPU max(1)[1]); decided on the values as given, no arithmetic."""
    return np.argmax(q, axis=1)


def head(W3, w4, q_np, q_nt, q_s, action, r_step, r_done, gamma, kind, delta, d1, hs, weights=None, dtype=np.float64, dq=None):
    """head_fused_kernel.  W3 [128,256], w4 [128], q_* [B,T], d1 [B,T,128], hs [B,T,256]; weights [B] = prioritized replay.  The expression
    shapes are the kernel's (dqn_head.h: dqn_dq, dqn_dq_w, dqn_loss_terms), so that dtype = float32 is the fp32 restatement.  dq given:
    the decoder part is computed from THAT dq (the GPU tests pass the kernel's own, to hold each stage to its own bound).
    Returns a dict; mag_loss / mag_db4 are the magnitudes their bounds scale with (absolute values of everything that enters)."""
    B, T = q_np.shape
    f = dtype
    am = first_argmax(q_np)
    a = np.clip(np.asarray(action, np.int64), 0, T - 1)
    rows = np.arange(B)
    qn, qsa = q_nt[rows, am].astype(f), q_s[rows, a].astype(f)
    rs, rd = r_step.astype(f) * f(0.1), r_done.astype(f) * f(0.1)
    y1, y2 = qn * f(gamma) + rs, rd
    e1, e2 = qsa - y1, qsa - y2
    w = np.ones(B, f) if weights is None else weights.astype(f)
    if kind == LOSS_HUBER:
        dl = f(delta)
        hub = lambda e: np.where(np.abs(e) < dl, f(0.5) * e * e, dl * (np.abs(e) - f(0.5) * dl))
        terms = hub(e1) + hub(e2)
        c, s = w * (f(1.0) / f(B)), np.clip(e1, -dl, dl) + np.clip(e2, -dl, dl)
    else:
        terms = e1 * e1 + e2 * e2
        c, s = w * (f(2.0) / f(B)), e1 + e2
    out = {"am": am, "a": a, "e1": e1, "e2": e2, "td": np.abs(e1) + np.abs(e2)}
    out["dq_own"] = c * s
    out["loss"] = (w * terms).sum(dtype=f) / f(B)
    out["db4"] = out["dq_own"].sum(dtype=f)
    m1 = np.abs(qsa) + np.abs(qn * f(gamma)) + np.abs(rs)
    m2 = np.abs(qsa) + np.abs(rd)
    out["mag_loss"] = float((np.abs(w) * (m1 * m1 + m2 * m2)).sum() / B)      # Huber's terms are below the squares
    out["mag_db4"] = float((np.abs(c) * (m1 + m2)).sum())
    d = out["dq_own"] if dq is None else np.asarray(dq).astype(f)
    d1r, hr = d1[rows, a].astype(f), hs[rows, a].astype(f)
    out["w4term"] = d[:, None] * d1r
    out["dd1c"] = np.where(d1r > 0, d[:, None] * w4.astype(f)[None], f(0))
    out["hcc"] = np.maximum(hr, 0)
    raw = out["dd1c"] @ W3.astype(f)
    out["dhc"] = np.where(hr > 0, raw, f(0))
    out["mag_dhc"] = np.abs(out["dd1c"]) @ np.abs(W3.astype(f))
    return out


HEAD_EXTRA = 8      # roundings of one row's loss term / dq before the batch sum (see head_bounds)


def head_bounds(ref, B):
    """loss and db4 are fp32 sums of B terms whose own arithmetic is not exact: y1 carries r*0.1f's rounding, the constant 0.1f's distance
    from 0.1 (a quarter ulp) and its addition's rounding, e1 = qsa - y1 one more - absolute errors against |qsa| + |qn gamma| + |0.1 r|, so the
    magnitudes are built from those sums -, squaring doubles that (7 half-ulps), the product, the two-term sum, the weight and the division
    by B add one each: under 8 ulps per term, and B - 1 additions on top.  (B + 8) 2^-23 mag covers it for every B >= 1."""
    return (B + HEAD_EXTRA) * U23 * ref["mag_loss"], (B + HEAD_EXTRA) * U23 * ref["mag_db4"]


def ulps32(got, want):
    """|got - want| in units of want's fp32 ulp (both float32 arrays)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ---------------------------------------------------------------- one BPTT pass
def bptt(whh, gates, cs, dhc, action, dtype=np.float64):
    """oracle.brain_oracle.brain_backward's recurrence (its lines 85-103) with a single loss frame per row: dL/dh enters direction d of row n
    at frame action[n] only.  whh [512,128], gates [2,N,T,512] (i, f, g, o after their activations), cs [2,N,T,128], dhc [N,256] ->
    dG [2,N,T,512], zero at the frames a direction consumes after the loss frame."""
    f = dtype
    whh, gates, cs, dhc = whh.astype(f), gates.astype(f), cs.astype(f), dhc.astype(f)
    _, N, T, _ = gates.shape
    a = np.clip(np.asarray(action, np.int64), 0, T - 1)
    dH = np.zeros((2, N, T, H), f)
    for d in range(2):
        dH[d, np.arange(N), a] = dhc[:, d * H:(d + 1) * H]
    dG = np.zeros((2, N, T, 4 * H), f)
    for d in range(2):
        dh_rec = np.zeros((N, H), f)
        dc = np.zeros((N, H), f)
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for s in range(T - 1, -1, -1):
            t = order[s]
            i, fg = gates[d, :, t, :H], gates[d, :, t, H:2 * H]
            g, o = gates[d, :, t, 2 * H:3 * H], gates[d, :, t, 3 * H:]
            c = cs[d, :, t]
            c_prev = cs[d, :, order[s - 1]] if s > 0 else np.zeros((N, H), f)
            tc = np.tanh(c)
            dh = dH[d, :, t] + dh_rec
            dc = dc + dh * o * (1 - tc * tc)
            dpre = np.concatenate([dc * g * i * (1 - i), dc * c_prev * fg * (1 - fg), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            dG[d, :, t] = dpre
            dh_rec = dpre @ whh
            dc = dc * fg
    return dG


def live_frames(action, N, T):
    """[2,N,T] bool: the frames direction d of row n consumes up to and including its loss frame (the others carry no gradient)."""
    a = np.clip(np.asarray(action, np.int64), 0, T - 1)
    t = np.arange(T)[None]
    return np.stack([t <= a[:, None], t >= a[:, None]])


def rel_err(x, ref64):
    """max |x - ref| relative to the tensor's largest element (the yardstick of test_bptt_error_against_fp64_is_in_the_class_of_torch_fp32)."""
    return float(np.abs(x.astype(np.float64) - ref64).max() / max(float(np.abs(ref64).max()), 1e-300))


# ---------------------------------------------------------------- the tail, composed as the step composes it
TAIL_KEYS = ("encoder_fc1.weight", "encoder_fc1.bias", "encoder_fc2.weight", "encoder_fc2.bias", "lstm_cell.weight_ih", "lstm_cell.weight_hh",
             "decoder_fc1.weight", "decoder_fc1.bias", "decoder_fc2.weight")
# (name, offset, shape) of the gradient arena, state_dict order (csrc/brain_fwd.h: O_W1 ...)
ARENA = (("encoder_fc1.weight", 0, (128, 2)), ("encoder_fc1.bias", 256, (128,)), ("encoder_fc2.weight", 384, (128, 128)),
         ("encoder_fc2.bias", 16768, (128,)), ("lstm_cell.weight_ih", 16896, (512, 128)), ("lstm_cell.weight_hh", 82432, (512, 128)),
         ("decoder_fc1.weight", 147968, (128, 256)), ("decoder_fc1.bias", 180736, (128,)), ("decoder_fc2.weight", 180864, (1, 128)),
         ("decoder_fc2.bias", 180992, (1,)))
NPARAMS = 180993


def tail_grads(dG, hprev, e, a1, dd1c, hcc, w4term, state, wih, w2, dtype=np.float64):
    """Everything behind the recurrence: dG [2,rows,512], hprev [2 rows,128], e, a1 [rows,128], dd1c, w4term [B,128], hcc [B,256],
    state [rows,2] -> (de, da1, {the nine gradient tensors the two tail launches and the reduction produce})."""
    rows = dG.shape[1]
    G = {}
    G["lstm_cell.weight_hh"] = wgrad(dG.reshape(2 * rows, 4 * H), None, hprev, dtype)
    G["lstm_cell.weight_ih"] = wgrad(dG[0], dG[1], e, dtype)
    G["decoder_fc1.weight"] = wgrad(dd1c, None, hcc, dtype)
    de, da1 = dgrad(dG[0], dG[1], wih, w2, a1, dtype)
    G["encoder_fc2.weight"] = wgrad(de, None, a1, dtype)
    G["encoder_fc2.bias"] = csum(de, None, dtype)[0]
    G["encoder_fc1.bias"], G["encoder_fc1.weight"] = csum(da1, state, dtype)
    G["decoder_fc2.weight"] = csum(w4term, None, dtype)[0][None]
    G["decoder_fc1.bias"] = csum(dd1c, None, dtype)[0]
    return de, da1, G


def tail_mags(dG, hprev, e, a1, dd1c, hcc, w4term, state, wih, w2):
    """The largest sum of absolute products behind any output of tail_grads: below 2^24 with integer operands, every fp32 partial sum of
    every kernel of the group is an exact integer in any order."""
    ab = lambda t: np.abs(np.asarray(t, np.float64))
    rows = dG.shape[1]
    de, da1 = dgrad(dG[0], dG[1], wih, w2, np.ones_like(a1))         # the values the later stages really sum (exact integers)
    dgx = ab(dG[0].astype(np.float64) + dG[1])
    mags = [dgx @ ab(wih), ab(de) @ ab(w2),                             # de, da1 (before its mask)
            ab(dG).reshape(2 * rows, -1).T @ ab(hprev), dgx.T @ ab(e), ab(dd1c).T @ ab(hcc),     # dW_hh, dW_ih, dW3
            ab(de).T @ ab(a1), ab(de).sum(0), ab(da1).sum(0), ab(da1).T @ ab(state),             # dW2, db2, db1, dW1
            ab(w4term).sum(0), ab(dd1c).sum(0)]                                                 # dW4, db3
    return max(float(m.max()) for m in mags)


# ---------------------------------------------------------------- fixtures
def ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


MASK_CLASSES = (np.float32(0.0), np.float32(-0.0), np.float32(-1.0), SUBNORMAL, np.float32(1.0))


def with_mask_classes(t, integer=False):
    """t with every mask class planted along its last axis, at positions that shift from row to row: +0, -0, a negative, the smallest
    positive subnormal, a positive.  integer = True leaves the subnormal out (it is no integer; the exact fixtures use the other four)."""
    t = np.array(t, np.float32)
    flat = t.reshape(-1, t.shape[-1])
    cls = [c for c in MASK_CLASSES if not (integer and c == SUBNORMAL)]
    for r in range(flat.shape[0]):
        for i, c in enumerate(cls):
            flat[r, (7 * r + 13 * i) % flat.shape[1]] = c
            flat[r, (7 * r + 13 * i + 64) % flat.shape[1]] = c
    return flat.reshape(t.shape)


def has_every_mask_class(t, integer=False):
    t = np.asarray(t, np.float32)
    z = t == 0
    ok = bool((t > 0).any() and (t < 0).any() and (z & ~np.signbit(t)).any() and (z & np.signbit(t)).any())
    return ok and (integer or bool((t == SUBNORMAL).any()))


# wgrad: (M, N, lda) with K and nslab from the lists below; lda > M reads A out of a wider buffer at column offset WG_COL0
WG_SHAPES = ((512, 128, 512), (128, 128, 128), (128, 256, 128), (128, 128, 512))
WG_COL0 = 64
WG_K1 = (1, 3, 15, 16, 17, 31, 33, 47, 48, 49, 63, 65, 95, 97, 143, 145)      # nslab = 1
WG_SPLITS = ((97, 2), (97, 3), (97, 7))
WG_AUTO = ((3225, 1), (6450, 0))                                                # (K, kind): the product's slab choice at B = 129, T = 25


def wgrad_fixture(M, N, K, has2, exact, seed=0):
    rng = np.random.default_rng([11, M, N, K, int(has2), int(exact), seed])
    if exact:
        return ints(rng, (K, M)), (ints(rng, (K, M)) if has2 else None), ints(rng, (K, N))
    n = lambda s: rng.standard_normal(s).astype(np.float32)
    return n((K, M)), (n((K, M)) if has2 else None), n((K, N))


DG_ROWS = (1, 15, 16, 17, 45, 129)


def dgrad_fixture(rows, exact):
    """-> dG, dG2 [rows,512], wih [512,128], w2 [128,128], a1 [rows,128] (a1 carries every mask class in every row)."""
    rng = np.random.default_rng([12, rows, int(exact)])
    if exact:
        return ints(rng, (rows, 512)), ints(rng, (rows, 512)), ints(rng, (512, 128)), ints(rng, (128, 128)), with_mask_classes(ints(rng, (rows, 128)), True)
    n = lambda s, k=1.0: (k * rng.standard_normal(s)).astype(np.float32)
    return n((rows, 512)), n((rows, 512)), n((512, 128), 0.1), n((128, 128), 0.1), with_mask_classes(n((rows, 128)))


CS_M = (1, 3, 7, 8, 9, 63, 64, 65, 121, 520)
CS_SPLITS = (1, 8)


def csum_fixture(M, N, with_x, exact):
    rng = np.random.default_rng([13, M, N, int(with_x), int(exact)])
    if exact:
        return ints(rng, (M, N), -8, 8), (ints(rng, (M, 2)) if with_x else None)
    n = lambda s: rng.standard_normal(s).astype(np.float32)
    return n((M, N)), (n((M, 2)) if with_x else None)


GROUP_BT = ((4, 3), (5, 9), (129, 25))


def group_fixture(B, T):
    """Integer operands for the whole tail: dG in {-1, 0, 1}, everything else in {-2 .. 2} (a1 with its mask classes)."""
    rng = np.random.default_rng([14, B, T])
    rows = B * T
    return dict(dG=ints(rng, (2, rows, 512), -1, 1), hprev=ints(rng, (2 * rows, 128)), e=ints(rng, (rows, 128)),
                a1=with_mask_classes(ints(rng, (rows, 128), -1, 1), True), dd1c=ints(rng, (B, 128)), hcc=ints(rng, (B, 256), 0, 2),
                w4term=ints(rng, (B, 128)), state=ints(rng, (rows, 2), -1, 1), wih=ints(rng, (512, 128), -1, 1), w2=ints(rng, (128, 128), -1, 1))


HEAD_B = (1, 2, 255, 256, 257)
HEAD_T = (1, 63, 64, 65)
HEAD_GAMMA = 0.75
HEAD_DELTA = 0.5


def head_cases():
    """(B, T, loss kind, prioritized): every B at T = 65 and every T at B = 2 and 257, both losses and both weightings spread over them, and
    the full cross of kind x weighting at (2, 65)."""
    cases = []
    for i, B in enumerate(HEAD_B):
        cases.append((B, 65, i % 2, (i // 2) % 2))
    for i, T in enumerate(HEAD_T):
        cases.append((2, T, (i + 1) % 2, i % 2))
        cases.append((257, T, i % 2, (i + 1) % 2))
    for kind in (0, 1):
        for per in (0, 1):
            cases.append((2, 65, kind, per))
    return sorted(set(cases))


def head_fixture(B, T):
    """Q values and weights on the 1/16 grid, gamma = 0.75, rewards zero or a power of two: qn * gamma and r * 0.1f are exact in fp32, so the
    fp32 restatement of e1 and e2 has ONE value whether or not the compiler contracts either product of y1 into its sum.  Row 0: maxima tied at the first and last frame; row 1: all frames equal; the
    rows after them tie at a middle frame and the last.  Rows 0 .. 2 (as far as B goes) with zero rewards and q_s, q_nt set for
    |e2| = delta with |e1| below, at and above it (delta = 0.5).  action alternates 0 / T - 1 / a middle frame; d1 and h carry every mask class."""
    rng = np.random.default_rng([15, B, T])
    g16 = lambda s, lo=-64, hi=64: (rng.integers(lo, hi + 1, size=s) / 16.0).astype(np.float32)
    q_np, q_nt, q_s = g16((B, T)), g16((B, T)), g16((B, T))
    action = np.array([(0, T - 1, T // 2)[b % 3] for b in range(B)], np.int64)
    for b in range(B):
        top = np.float32(5.0)
        if b == 0:
            q_np[b, 0] = q_np[b, T - 1] = top
        elif b == 1:
            q_np[b, :] = np.float32(0.25)
        else:
            q_np[b, (b * 7) % T] = q_np[b, T - 1] = top
    pow2 = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], np.float32)
    r_step, r_done = pow2[rng.integers(0, 9, B)], pow2[rng.integers(0, 9, B)]
    am = first_argmax(q_np)
    for b, qn in zip(range(min(B, 3)), (0.5, 0.0, 2.0)):        # e2 = q_s = delta; e1 = delta - 0.75 qn = 0.125, 0.5, -1.0
        r_step[b] = r_done[b] = 0.0
        q_s[b, np.clip(action[b], 0, T - 1)] = HEAD_DELTA
        q_nt[b, am[b]] = qn
    weights = g16((B,), 1, 32)
    W3 = (0.1 * rng.standard_normal((128, 256))).astype(np.float32)
    w4 = (0.1 * rng.standard_normal(128)).astype(np.float32)
    d1 = with_mask_classes(rng.standard_normal((B, T, 128)).astype(np.float32))
    hs = with_mask_classes(rng.standard_normal((B, T, 256)).astype(np.float32))
    if B > 3:
        d1[3, np.clip(action[3], 0, T - 1)] = -np.abs(d1[3, np.clip(action[3], 0, T - 1)])      # a row whose dd1 is all zeros
    return dict(W3=W3, w4=w4, q_np=q_np, q_nt=q_nt, q_s=q_s, action=action, r_step=r_step, r_done=r_done, weights=weights, d1=d1, hs=hs)


LSTM_N = {0: (1, 3), 1: (1, 3), 2: (1, 3, 130), 4: (1, 3, 130)}      # form -> batch sizes
LSTM_T = (1, 2, 9)


def lstm_fixture(N, T):
    """Activations as a forward leaves them (sigmoid / tanh of unit-normal pre-activations, cell states of that scale), W_hh in torch's
    default range, action cycling over frame 0, T - 1 and a middle frame - with N = 130 the rows of a workgroup stop at different steps."""
    rng = np.random.default_rng([16, N, T])
    pre = rng.standard_normal((2, N, T, 4 * H))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    gates = np.concatenate([sig(pre[..., :2 * H]), np.tanh(pre[..., 2 * H:3 * H]), sig(pre[..., 3 * H:])], -1).astype(np.float32)
    cs = (0.7 * rng.standard_normal((2, N, T, H))).astype(np.float32)
    s = 1.0 / np.sqrt(H)
    whh = rng.uniform(-s, s, (4 * H, H)).astype(np.float32)
    dhc = (0.1 * rng.standard_normal((N, 2 * H))).astype(np.float32)
    action = np.array([(0, T - 1, T // 2, min(1, T - 1))[n % 4] for n in range(N)], np.int64)
    return dict(whh=whh, gates=gates, cs=cs, dhc=dhc, action=action)


# ================================================================ the Brain forward (tests/test_gpu_dqn_fwd_kernels.py)
# Float64 restatements of enc_fused_kernel, dec_fused_kernel (csrc/brain_fused.h), the recurrence forms and brain_fwd_mega_kernel
# (csrc/lstm_fwd.h), their error bounds and their fixtures.  P is a dict of the ten state_dict tensors (SHAPES below); arena(P) lays it out
# as the kernels read it.  tests/test_dqn_ref.py pins the composition enc -> lstm_fwd -> dec to oracle.brain_oracle.brain_forward.
SHAPES = {name: shape for name, _, shape in ARENA}
LOG2E32 = np.float32(1.4426950408889634)


def arena(P):
    """The fp32 parameter arena (state_dict order) of a parameter dict."""
    flat = np.zeros(NPARAMS, np.float32)
    for name, off, shape in ARENA:
        flat[off:off + int(np.prod(shape))] = np.asarray(P[name], np.float32).reshape(-1)
    return flat


def enc(P, x, dtype=np.float64):
    """x [rows,2] -> a1 = relu(x W1^T + b1), e = a1 W2^T + b2, gx = e W_ih^T."""
    f = dtype
    a1 = np.maximum(x.astype(f) @ P["encoder_fc1.weight"].astype(f).T + P["encoder_fc1.bias"].astype(f), 0)
    e = a1 @ P["encoder_fc2.weight"].astype(f).T + P["encoder_fc2.bias"].astype(f)
    return a1, e, e @ P["lstm_cell.weight_ih"].astype(f).T


def enc_bounds(P, x):
    """Per-element bounds of (a1, e, gx) against enc in float64: each stage an fp32 sum of K products (and a bias) in any order,
    (K + 2) 2^-23 sum |a||b|, on ITS input - within the previous stage's bound of the reference's -, plus that bound carried through |W|.
    relu moves nothing by more than its argument moved."""
    ab = lambda k: np.abs(np.asarray(P[k], np.float64))
    a1, e, _ = enc(P, x)
    b_a1 = sum_bound(2, np.abs(x.astype(np.float64)) @ ab("encoder_fc1.weight").T + ab("encoder_fc1.bias"))
    w2 = ab("encoder_fc2.weight").T
    b_e = sum_bound(128, (a1 + b_a1) @ w2 + ab("encoder_fc2.bias")) + b_a1 @ w2
    wih = ab("lstm_cell.weight_ih").T
    return b_a1, b_e, sum_bound(128, (np.abs(e) + b_e) @ wih) + b_e @ wih


def dec(P, hs, dtype=np.float64):
    """hs [rows,256] -> d1 = relu(relu(hs) W3^T + b3), q = d1 w4 + b4."""
    f = dtype
    d1 = np.maximum(np.maximum(hs.astype(f), 0) @ P["decoder_fc1.weight"].astype(f).T + P["decoder_fc1.bias"].astype(f), 0)
    return d1, d1 @ P["decoder_fc2.weight"].astype(f)[0] + P["decoder_fc2.bias"].astype(f)[0]


def dec_bounds(P, hs):
    """(bound of d1, bound of q): K = 256 on relu(hs), then K = 128 on the kernel's own d1 plus d1's bound carried through |w4|."""
    ab = lambda k: np.abs(np.asarray(P[k], np.float64))
    d1, _ = dec(P, hs)
    b_d1 = sum_bound(256, np.maximum(hs.astype(np.float64), 0) @ ab("decoder_fc1.weight").T + ab("decoder_fc1.bias"))
    w4 = ab("decoder_fc2.weight")[0]
    return b_d1, sum_bound(128, (d1 + b_d1) @ w4 + ab("decoder_fc2.bias")[0]) + b_d1 @ w4


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_step(whh, gx_t, hprev, cprev, dtype=np.float64):
    """One frame of the cell: gx_t [..,512], hprev, cprev [..,128] -> (gates [..,512] after their activations (i, f, g, o), c, h)."""
    f = dtype
    pre = gx_t.astype(f) + hprev.astype(f) @ whh.astype(f).T
    gates = np.concatenate([_sig(pre[..., :2 * H]), np.tanh(pre[..., 2 * H:3 * H]), _sig(pre[..., 3 * H:])], -1).astype(f)
    c = gates[..., H:2 * H] * cprev.astype(f) + gates[..., :H] * gates[..., 2 * H:3 * H]
    return gates, c, gates[..., 3 * H:] * np.tanh(c)


def prev_frame(d, t):
    """The frame direction d consumed before frame t (-1 / T: none)."""
    return t - 1 if d == 0 else t + 1


def lstm_fwd(whh, gx, dtype=np.float64):
    """Both directions from a zero state: gx [N,T,512] -> hs [N,T,256] (h_fw | h_bw after frame t), gates [2,N,T,512], cs, hprev [2,N,T,128]
    (hprev: h before the frame), in the layouts the kernels write."""
    f = dtype
    N, T, _ = gx.shape
    hs, gates = np.zeros((N, T, 2 * H), f), np.zeros((2, N, T, 4 * H), f)
    cs, hprev = np.zeros((2, N, T, H), f), np.zeros((2, N, T, H), f)
    for d in range(2):
        h, c = np.zeros((N, H), f), np.zeros((N, H), f)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            hprev[d, :, t] = h
            gates[d, :, t], c, h = lstm_step(whh, gx[:, t], h, c, f)
            cs[d, :, t], hs[:, t, d * H:(d + 1) * H] = c, h
    return hs, gates, cs, hprev


# ---- the device's activation expressions in fp32 numpy (common.h: fast_exp, fast_rcp, fast_tanh; lstm_fwd_*: sg, act)
def _fma32(a, b, c):
    """fl32(a b + c) for fp32 a, c and b in {1, 2}: the product is exact in float64 and so is the sum of two fp32 numbers of this range."""
    return (a.astype(np.float64) * b + c).astype(np.float32)


def gate_act32(pre, gk):
    """x log2e -> exp2 -> 1 + . -> reciprocal -> fma(sg, gk, 1 - gk) with x = -gk pre: the sigmoid (gk = 1) and, as 2 sigmoid(2x) - 1, the tanh
    (gk = 2) of the gate pre-activations, every operation rounded to fp32."""
    pre = np.asarray(pre, np.float32)
    g = np.float32(gk)
    with np.errstate(over="ignore"):
        sg = np.float32(1.0) / (np.float32(1.0) + np.exp2((-g * pre) * LOG2E32, dtype=np.float32))
    return _fma32(sg, float(gk), 1.0 - float(gk))


def cell_tanh32(c):
    """1 - 2 rcp(exp2(2c log2e) + 1), every operation rounded to fp32."""
    c = np.asarray(c, np.float32)
    with np.errstate(over="ignore"):
        r = np.float32(1.0) / (np.exp2((np.float32(2.0) * c) * LOG2E32, dtype=np.float32) + np.float32(1.0))
    return np.float32(1.0) - np.float32(2.0) * r


ACT_MARGIN = 4      # v_exp_f32 and v_rcp_f32 may each be an ulp off where numpy rounds correctly


def act_terms(whh, gx):
    """The activation allowances of the step check, from the fixture alone (never from device output): ACT_MARGIN x the worst error against
    float64 of the fp32 restatements above over the float64 chain's own pre-activations and cell states.  -> (sigmoid gates, g gate, tanh(c))."""
    N, T, _ = gx.shape
    _, gates, cs, hprev = lstm_fwd(whh, gx)
    pre = gx.astype(np.float64)[None] + hprev @ whh.astype(np.float64).T
    sgm = np.concatenate([pre[..., :2 * H], pre[..., 3 * H:]], -1)
    e_s = np.abs(gate_act32(sgm, 1).astype(np.float64) - _sig(sgm.astype(np.float32).astype(np.float64))).max()
    g = pre[..., 2 * H:3 * H]
    e_g = np.abs(gate_act32(g, 2).astype(np.float64) - np.tanh(g.astype(np.float32).astype(np.float64))).max()
    e_c = np.abs(cell_tanh32(cs).astype(np.float64) - np.tanh(cs.astype(np.float32).astype(np.float64))).max()
    return ACT_MARGIN * float(e_s), ACT_MARGIN * float(e_g), ACT_MARGIN * float(e_c)


def _peak_slope(kind, x, r):
    """The largest slope of sigmoid (kind 0) or tanh (kind 1) on [x - r, x + r]: both slopes peak at 0 and fall off monotonically."""
    z = np.where(np.abs(x) <= r, 0.0, np.abs(x) - r)
    if kind == 0:
        s = _sig(z)
        return s * (1 - s)
    return 1 - np.tanh(z) ** 2


def step_bounds(whh, gx_t, hprev, cprev, acts):
    """Allowances of (gates, c, h) of ONE step against lstm_step in float64 on the same gx_t, hprev, cprev.  The pre-activation is an fp32
    sum of 128 products and gx_t in any order: lin = (128 + 2) 2^-23 (sum |h||w| + |gx_t|); a gate moves by at most the activation's largest
    slope within lin of the reference's pre-activation times lin, plus the activation term of act_terms.  c = f c' + i g and h = o tanh(c)
    carry the gates' allowances through their factors and add 2^-23 of each rounded product and sum."""
    a_s, a_g, a_c = acts
    w = np.abs(whh.astype(np.float64))
    pre = gx_t.astype(np.float64) + hprev.astype(np.float64) @ whh.astype(np.float64).T
    lin = sum_bound(128, np.abs(hprev.astype(np.float64)) @ w.T + np.abs(gx_t.astype(np.float64)))
    kind = np.zeros(4 * H, np.int64)
    kind[2 * H:3 * H] = 1
    slope = np.where(kind == 1, _peak_slope(1, pre, lin), _peak_slope(0, pre, lin))
    b_g = slope * lin + np.where(kind == 1, a_g, a_s)
    gates, c, h = lstm_step(whh, gx_t, hprev, cprev)
    i, fg, g, o = (np.abs(gates[..., k * H:(k + 1) * H]) for k in range(4))
    bi, bf, bg, bo = (b_g[..., k * H:(k + 1) * H] for k in range(4))
    cp = np.abs(cprev.astype(np.float64))
    b_c = cp * bf + (g + bg) * bi + i * bg + 2 * U23 * (fg * cp + i * g)
    tc = np.abs(np.tanh(c))
    b_h = tc * bo + (o + bo) * (_peak_slope(1, c, b_c) * b_c + a_c) + U23 * np.abs(h)
    return b_g, b_c, b_h


# ---- fixtures of the forward tests
ENC_ROWS = (1, 47, 48, 49, 97)


def enc_cases(rows):
    """(rows0, keep_row) of the table: the x / x2 boundary at rows (no x2), inside the second tile and after the first row; the kept rows from
    0, from inside the second tile, and none."""
    return [(r0, k) for r0 in sorted({rows, 50, 1}, reverse=True) if r0 <= rows for k in sorted({0, 50, rows}) if k <= rows]


TWO_JOBS = ((49, 1, 48), (47, 47, 0))       # (rows, rows0, keep_row) of the two-job cases: job 0, job 1 (its tiles start at workgroup 2)


def _edge_rows(x):
    """The relu's edge in the input: rows of +0, -0, negatives and the smallest subnormal of either sign, from the last row backwards (every
    tile shape has its tail rows among them), as many as fit."""
    edge = np.array([[0.0, 0.0], [-0.0, -0.0], [-1.0, -2.0], [SUBNORMAL, 0.0], [0.0, -SUBNORMAL], [-SUBNORMAL, SUBNORMAL]], np.float32)
    n = min(len(edge), x.shape[0])
    x[x.shape[0] - n:] = edge[:n] if x.shape[0] >= len(edge) else edge[[3, 1, 0, 2, 4, 5][:n]]
    return x


def brain_params(seed, exact):
    """A parameter dict.  exact: W1, b1 in {-2 .. 2} with b1 nowhere 0 (a subnormal input is absorbed: a1 stays an integer), W2, b2, W_ih in
    {-1, 0, 1}, W3, w4, b3, b4 in {-1, 0, 1}.  dense: torch's default ranges; units 0 .. 3 of encoder_fc1 have b1 = 0 and the weight rows
    (1, 0), (-1, 0), (0, 1), (0, -1), so that their pre-activation IS +-x: the relu sees +0, -0 and +-subnormal exactly."""
    rng = np.random.default_rng([21, seed, int(exact)])
    P = {}
    for name, _, shape in ARENA:
        if exact:
            P[name] = ints(rng, shape, -1, 1)
        else:
            s = 1.0 / np.sqrt(shape[-1] if len(shape) > 1 else 128)
            P[name] = rng.uniform(-s, s, shape).astype(np.float32)
    if exact:
        P["encoder_fc1.weight"] = ints(rng, (128, 2))
        b1 = ints(rng, (128,))
        P["encoder_fc1.bias"] = np.where(b1 == 0, np.float32(1.0), b1).astype(np.float32)
    else:
        P["encoder_fc1.weight"][:4] = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)
        P["encoder_fc1.bias"][:4] = 0.0
    return P


def enc_fixture(rows, exact, seed=0):
    """x [rows,2]: integers in {-2 .. 2} (exact) or uniform in [0, 1) as the states are (dense), with the edge rows of _edge_rows."""
    rng = np.random.default_rng([22, rows, int(exact), seed])
    x = ints(rng, (rows, 2)) if exact else rng.uniform(0, 1, (rows, 2)).astype(np.float32)
    return _edge_rows(x)


def dec_fixture(rows, exact, seed=0):
    """hs [rows,256] with the mask classes in every row: integers in {-2 .. 2} (exact; the subnormal is no integer and stays out) or
    uniform in (-1, 1) as h is (dense, all five classes)."""
    rng = np.random.default_rng([23, rows, int(exact), seed])
    if exact:
        return with_mask_classes(ints(rng, (rows, 256)), True)
    return with_mask_classes(rng.uniform(-1, 1, (rows, 256)).astype(np.float32))


FWD_T = (1, 2, 3, 9)
FORM_MFMA = 20
FWD_FORMS_SMALL = (1, 2, 4, 11, 12, 14)                      # lstm_fwd_kernel<R>, lstm_fwd_quad_kernel<R> (10 + R): N in FWD_N_SMALL
FWD_N_SMALL, FWD_N_MFMA = (1, 3), (4, 5, 6)
FORM_NAMES = {1: "plain<1>", 2: "plain<2>", 4: "plain<4>", 11: "quad<1>", 12: "quad<2>", 14: "quad<4>", 20: "mfma"}
RAGGED_LENGTHS = (1, 2, 9, 1)
MEGA_T = (1, 32, 33)


def product_form(N):
    """The recurrence form the forward drivers choose at N samples with the default tunables (csrc/brain.hip: lstm_fwd_form_for)."""
    rows = 2 * N
    return FORM_MFMA if rows >= 8 else 10 + (1 if rows <= 256 else 2 if rows <= 512 else 4)


def fwd_fixture(N, T, seed=0):
    """whh in torch's default range, gx [N,T,512] unit normal (the scale W_ih e has on trained weights)."""
    rng = np.random.default_rng([24, N, T, seed])
    s = 1.0 / np.sqrt(H)
    return rng.uniform(-s, s, (4 * H, H)).astype(np.float32), rng.standard_normal((N, T, 4 * H)).astype(np.float32)


def saturating_fixture(N, T):
    """gx = +-100 with every combination of the four gates' signs (unit j of sample n at frame t: combination (j + n + t) mod 16)."""
    whh, _ = fwd_fixture(N, T, 1)
    j = np.arange(H)[None, None, :] + np.arange(N)[:, None, None] + np.arange(T)[None, :, None]
    gx = np.concatenate([np.where((j >> k) & 1, 100.0, -100.0) for k in range(4)], -1).astype(np.float32)
    return whh, gx
