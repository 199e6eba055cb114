"""One ResNet bottleneck block restated in plain torch on the CPU, as the fused bf16 kernels of csrc/bottleneck.hip and
csrc/bottleneck_wide.hip compute it, plus the fixtures and bounds that tests/test_gpu_bneck_kernels.py holds those kernels to
(tools/bneck_probe.py and tools/bneck_wide_probe.py print the same figures).  No GPU is needed for anything in this file.

Layout (the probes' own, include/ivosw_probe.h): x [B,H,W,Cin] NHWC; wa [Cmid,Cin]; wb [Cmid, 3*3*Cmid] with K = (ky*3 + kx)*Cmid + c;
wc [4*Cmid,Cmid]; optional wd [4*Cmid,Cin]; fp32 biases.  Operands are bf16 values, widened.

    t1  = bf16_rne(relu(conv1x1(x, wa) + ba))
    t2  = bf16_rne(relu(conv3x3(t1, wb, pad 1) + bb))
    pre = relu(conv1x1(t2, wc) + bc + (conv1x1(x, wd) + bd  if wd  else  x))

`block` returns pre UNROUNDED (the kernels' output is bf16_rne(pre)).  The rounding points are those of the kernels' epilogues, read
from the sources: t1 and t2 leave their fp32 accumulators through pack2_bf16 (round to nearest even, v_cvt_pk_bf16_f32) after bias
and ReLU; conv3's fp32 accumulator takes its bias and the widened bf16 residual (or, in bneck64_kernel<64, true>, the downsample's
products in the same accumulator and both biases) in fp32 BEFORE the one rounding of the output.  The wide kernels round first and
apply the ReLU to the packed pair (relu2_bf16): the same bits, since rounding is monotonic and keeps the sign.  No kernel rounds
anywhere else, so nothing here deviates from the three lines above.
"""
import functools

import torch

NAN_BITS = 0x7FA5          # a bf16 NaN as int16: what the tests pre-fill y and its guard frames with


def bf16_rne(t):
    """Round to the nearest bf16 value, ties to even, staying in t's dtype.  float64 is rounded on its own bits (through float32 it
    would be rounded twice); the values of this file are far from bf16's exponent limits."""
    if t.dtype == torch.float64:
        u = t.contiguous().view(torch.int64)
        u = u + ((1 << 44) - 1) + ((u >> 45) & 1)          # 52 - 7 = 45 mantissa bits go
        return (u & ~((1 << 45) - 1)).view(torch.float64)
    return t.to(torch.bfloat16).to(t.dtype)


def _taps(t):
    """[B,H,W,C] -> [B,H,W,9*C]: the 3 x 3 neighbourhood with zero padding, K = (ky*3 + kx)*C + c."""
    B, H, W, C = t.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=t.dtype)
    p[:, 1:-1, 1:-1] = t
    return torch.cat([p[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=-1)


def block(x, wa, ba, wb, bb, wc, bc, wd=None, bd=None, dtype=torch.float64, parts=False):
    """The block above with every product, sum and bias in `dtype`.  parts=True also returns t1, t2, their unrounded values before
    the ReLU, and per layer the sum of |terms| of every output (what the fixtures themselves are checked on)."""
    c = lambda t: None if t is None else t.to(dtype)
    x, wa, ba, wb, bb, wc, bc, wd, bd = map(c, (x, wa, ba, wb, bb, wc, bc, wd, bd))
    a1 = x @ wa.t() + ba
    t1 = bf16_rne(torch.relu(a1))
    k2 = _taps(t1)
    a2 = k2 @ wb.t() + bb
    t2 = bf16_rne(torch.relu(a2))
    idt = x @ wd.t() + bd if wd is not None else x
    pre = torch.relu(t2 @ wc.t() + bc + idt)
    if not parts:
        return pre
    m1 = x.abs() @ wa.abs().t() + ba.abs()
    m2 = k2.abs() @ wb.abs().t() + bb.abs()
    m3 = t2.abs() @ wc.abs().t() + bc.abs() + (x.abs() @ wd.abs().t() + bd.abs() if wd is not None else x.abs())
    return pre, {"a1": a1, "a2": a2, "t1": t1, "t2": t2, "mag": (m1, m2, m3)}


def ref64(x, wa, ba, wb, bb, wc, bc, wd=None, bd=None):
    return block(x, wa, ba, wb, bb, wc, bc, wd, bd, dtype=torch.float64)


def ref32(x, wa, ba, wb, bb, wc, bc, wd=None, bd=None):
    """The same in float32, in whatever order torch's CPU kernels sum: ONE legitimate fp32 ordering, the yardstick of the dense bound."""
    return block(x, wa, ba, wb, bb, wc, bc, wd, bd, dtype=torch.float32)


# ---------------------------------------------------------------- the cases: (entry, Cin, Cmid, H) and the frame counts of each
# entry "b": ivosw_bneck_probe, "w": ivosw_bneck_wide_probe; H = W is the smallest each kernel accepts
SHAPES = {
    "id64":  ("b", 256, 64, (1, 16), (3, 32)),           # bneck64_kernel<256,false>: one tile (every border padded) | 2 x 2 tiles, 3 frames
    "ds64":  ("b", 64, 64, (1, 16), (2, 32)),            # bneck64_kernel<64,true>: wd / bd
    "res2":  ("w", 256, 64, (1, 64), (2, 64)),
    "res3":  ("w", 512, 128, (1, 32), (3, 32)),
    "res4":  ("w", 1024, 256, (1, 16), (3, 16)),
    "res5":  ("w", 2048, 512, (1, 8), (2, 8), (3, 8), (4, 8)),
}


def shape_cases():
    return [(name, B, H) for name, s in SHAPES.items() for B, H in s[3:]]


def _signs(n, g):
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


def _sparse(rows, K, cols, g):
    """[rows,K] with entries in {-1,0,+1}: row r has a nonzero at every column cols(r, j); random signs, cyclic places."""
    w = torch.zeros(rows, K)
    for r in range(rows):
        c = torch.tensor(cols(r))
        assert len(set(c.tolist())) == len(c)
        w[r, c] = _signs(len(c), g)
    return w


@functools.lru_cache(maxsize=None)
def exact_fixture(name, B, H):
    """Small integers throughout, so that no summation order can change a bit (test_bneck_ref.py checks the conditions on ref64's own
    intermediates): x in [-3,3] on even and [-1,2] on odd channels, random per element; 8 nonzeros per wa / wc / wd row, 9 per wb row
    (one per tap), placed cyclically so that every K index of every layer meets a nonzero and every row has one."""
    _, Cin, Cm, *_ = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * Cin + 10 * H + B)
    x = torch.randint(-3, 4, (B, H, H, Cin), generator=g).float()
    x[..., 1::2] = torch.randint(-1, 3, (B, H, H, Cin // 2), generator=g).float()
    wa = _sparse(Cm, Cin, lambda r: [(r + j * (Cin // 8)) % Cin for j in range(8)], g)
    wb = _sparse(Cm, 9 * Cm, lambda r: [j * Cm + (3 * r + 11 * j + 1) % Cm for j in range(9)], g)
    wc = _sparse(4 * Cm, Cm, lambda r: [(5 * r + j * (Cm // 8) + r // Cm) % Cm for j in range(8)], g)
    ba = torch.randint(-2, 3, (Cm,), generator=g).float()
    bb = torch.randint(-3, 4, (Cm,), generator=g).float()
    bc = torch.randint(-4, 5, (4 * Cm,), generator=g).float()
    wd = bd = None
    if Cin != 4 * Cm:
        wd = _sparse(4 * Cm, Cin, lambda r: [(3 * r + j * (Cin // 8) + r // Cin) % Cin for j in range(8)], g)
        bd = torch.randint(-2, 3, (4 * Cm,), generator=g).float()
    return x, wa, ba, wb, bb, wc, bc, wd, bd


# d32 = max |ref32 - ref64| is to measure what ONE legitimate fp32 reordering costs: a t1 value whose bf16 rounding flips (about one
# in 10^4), the t2 flips that follow it, and what they do to the output.  It is the maximum of that process only if the sample holds
# flips at all: one 16 x 16 frame of 64 channels has 16 k t1 values, one res4 frame 65 k, and there ref32 and ref64 often agree on every
# one of them (d32 = 1e-4 ... 1e-5, fp32 noise; WHICH frames depends on the host's sgemm) while the kernel, summing in its own order,
# flips another value.  So the two references are taken over a batch of dense_frames() frames of one recipe, at least 2^19 t1 values,
# d32 is their maximum over that whole batch, and a kernel case of B frames runs on the first B of them (frames are independent of each
# other in every kernel).  m32 and every comparison with y use those B frames only.
DENSE_T1 = 1 << 19


def dense_frames(name, H):
    return max(max(B for B, h in SHAPES[name][3:] if h == H), -(-DENSE_T1 // (H * H * SHAPES[name][2])))


@functools.lru_cache(maxsize=None)
def dense_fixture(name, H):
    """The probe tools' recipe - randn activations, randn / sqrt(K) weights, 0.1 * randn biases, rounded to bf16 - scaled per channel
    (as test_big_register_tile_contraction_vs_torch scales its rows) so that a swapped channel or row is not statistically invisible.
    x holds dense_frames(name, H) frames."""
    _, Cin, Cm, *_ = SHAPES[name]
    B = dense_frames(name, H)
    g = torch.Generator().manual_seed(2000 * Cin + 10 * H)
    r16 = lambda t: t.to(torch.bfloat16).float()

    def w(rows, K):
        return r16(torch.randn(rows, K, generator=g) / K ** 0.5 * (1 + torch.arange(rows)[:, None] % 5 * 0.5))
    x = r16(torch.randn(B, H, H, Cin, generator=g) * (1 + torch.arange(Cin) % 7 * 0.25))
    wa, wb, wc = w(Cm, Cin), w(Cm, 9 * Cm), w(4 * Cm, Cm)
    ba, bb, bc = (0.1 * torch.randn(n, generator=g) for n in (Cm, Cm, 4 * Cm))
    wd = bd = None
    if Cin != 4 * Cm:
        wd, bd = w(4 * Cm, Cin), 0.1 * torch.randn(4 * Cm, generator=g)
    return x, wa, ba, wb, bb, wc, bc, wd, bd


@functools.lru_cache(maxsize=None)
def exact_want(name, B, H):
    """bf16_rne(ref64) of the exact fixture as float32: what the kernel's output must equal bit for bit."""
    return bf16_rne(ref64(*exact_fixture(name, B, H))).float() + 0.0


def bounds(r64, r32):
    """The dense fixture's two yardsticks, from the references alone: d32 = max |ref32 - ref64|, m32 = mean |bf16_rne(ref32) - ref64|."""
    return float((r32.double() - r64).abs().max()), float((bf16_rne(r32).double() - r64).abs().mean())


def figures(y, r64, d32, m32):
    """The kernel's two figures against the two bounds: every element within 2^-8 |ref64| (the output's own bf16 rounding) + 4 * d32
    (one legitimate fp32 reordering, margin 4), and mean |y - ref64| within 1.5 * m32.  Returns (worst element error over its bound,
    mean error, d32, m32): the bounds hold iff ratio <= 1 and mean <= 1.5 * m32."""
    err = (y.double() - r64).abs()
    return float((err / (r64.abs() * 2.0 ** -8 + 4 * d32)).max()), float(err.mean()), d32, m32


def report(y, fx):
    """For the probe tools: one line with the figures of y (CPU, [B,H,W,4*Cmid]) on the operands fx (CPU, in the order of `block`)."""
    r64, r32 = ref64(*fx), ref32(*fx)
    ratio, mean, d32, m32 = figures(y, r64, *bounds(r64, r32))
    return (f"vs the fp64 restatement (tests/bneck_ref.py): d32 {d32:.3e}  m32 {m32:.3e}  worst |y-ref64| / (2^-8 |ref64| + 4 d32) = {ratio:.3f}  "
            f"mean |y-ref64| = {mean:.3e} = {mean / m32:.3f} m32   [bounds: <= 1, <= 1.5]")


def dense_case(name, B, H):
    """The operands of a kernel case: the first B frames of the shape's dense batch."""
    fx = dense_fixture(name, H)
    return (fx[0][:B].contiguous(),) + fx[1:]


@functools.lru_cache(maxsize=None)
def dense_refs(name, H):
    """(ref64, ref32, d32) over the shape's whole dense batch, computed once and shared by every frame count and arm."""
    fx = dense_fixture(name, H)
    r64, r32 = ref64(*fx), ref32(*fx)
    return r64, r32, bounds(r64, r32)[0]


def dense_figures(y, name, B, H):
    r64, r32, d32 = dense_refs(name, H)
    return figures(y, r64[:B], d32, bounds(r64[:B], r32[:B])[1])
