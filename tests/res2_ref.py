"""res2 with res3's forwarded conv1 (csrc/res2_chain.hip, csrc/res2_stage.hip) and the fused stem (stem_pool_kernel, csrc/stem.hip) restated
in plain torch on the CPU, with the fixtures, bounds and case tables that tests/test_gpu_res2_stem_kernels.py holds those kernels to, each
launched alone through ivosw_res2_probe / ivosw_stem_probe (include/ivosw_probe.h).  tests/test_res2_ref.py pins this file on the CPU.  No
GPU is needed for anything in it.

res2.  x [B,64,64,64] NHWC; eleven K-major weights and fp32 biases in the probe's order (W_NAMES): conv1 of res2's three blocks and of
res3's first block, conv2 x 3 (K = (ky*3 + kx)*64 + c), conv3 x 3, block 0's downsample.  Operands are bf16 values, widened.

    y0    = bf16_rne(bneck_ref.block(x,  w1_0, b1_0, w2_0, b2_0, w3_0, b3_0 (+) bd, wd, 0))      [conv3 | downsample]: ONE fp32 sum
    y1    = bf16_rne(bneck_ref.block(y0, w1_1, b1_1, w2_1, b2_1, w3_1, b3_1))                     identity blocks: + the bf16 input
    y2    = bf16_rne(bneck_ref.block(y1, w1_2, b1_2, w2_2, b2_2, w3_2, b3_2))
    t1out = bf16_rne(relu(y2 @ w1_3^T + b1_3))
    y     = y2, or with y_s2 its even pixels y2[:, ::2, ::2]

`res2` returns y2 and t1out UNROUNDED (the kernels' outputs are bf16_rne of them).  The rounding points, read from the sources: both kernels
round t1, t2, y and t1out exactly once each.  res2_chain.hip: store_t1 (relu2_bf16 of the fp32 accumulator, frame mask) for every t1; epi_t2
and epi_y / epi_yq (relu2_bf16) for t2 and y - the packed y IS the next conv1's operand and, through the identity fragments `idf`, the next
block's residual, so the residual is the rounded value; the last lines of block 2 (relu2_bf16 of acc) for t1out.  res2_stage.hip: A0's
epilogue and store_t1 for t1; phase_b's exchange epilogue for t2 (both K halves and the bias are added in fp32 first); finish_c for y (bias
as the initial accumulator, the widened bf16 residual added in fp32, one relu2_bf16; the LDS image that feeds phase D and the registers that
carry the residual hold the same packed value); D2's epilogue for t1out.  Block 0 has no residual: the downsample's products join conv3's in
one fp32 accumulator.  relu2_bf16 rounds first and applies the ReLU to the packed pair: the same bits, rounding is monotonic and keeps the
sign.  t1 outside the 64 x 64 frame is the 3x3's zero padding (the frame masks of store_t1), not relu(bias): `bneck_ref._taps` pads with 0.

Biases.  form 0 (res2_stage_kernel) adds the fp32 bias; block 0's conv3 takes fp32(b3 + bd), the sum launch_concat_k makes.  form 1
(res2_chain_kernel) adds a bias as one MFMA against the (hi, lo) bf16 split res2_chain_pack_kernel makes of the fp32 value b:
hi = bf16(b), lo = bf16(b - hi), so what enters the sum is hi + lo (exact in fp32: both halves lie within b's 24 bits), NOT b; for block 0's
conv3 b = fp32(b3 + bd).  `kernel_biases` gives the values of either form and `res2(form=...)` uses them.

stem.  roi [B,256,256,4]; w [64, 7*7*4] with K = (ky*7 + kx)*4 + c; fp32 bias [64].

    c   = bf16_rne(relu(conv7x7 stride 2 pad 3 (roi, w) + bias))          [B,128,128,64]
    out = maxpool 3x3 stride 2 pad 1 (c)                                   [B,64,64,64]; positions outside the 128 x 128 map take no part

`stem` returns the maximum of the UNROUNDED relu values: rounding before or after the maximum gives the same bits (monotonic).  The kernel
starts its accumulator from the fp32 bias, rounds once (relu2_bf16), zeroes the positions outside the map (all values are >= 0, so a zero
never wins against a position inside) and takes the maximum on the packed u16 patterns (order-preserving for non-negative bf16).
"""
import collections
import functools

import torch

from tests import bneck_ref as BR
from tests.bneck_ref import DENSE_T1, NAN_BITS, _sparse, bf16_rne, bounds, figures  # noqa: F401  (re-exported for the tests)

W_NAMES = ("w1_0", "w1_1", "w1_2", "w1_3", "w2_0", "w2_1", "w2_2", "w3_0", "w3_1", "w3_2", "wd")
W_SHAPES = ((64, 64), (64, 256), (64, 256), (128, 256), (64, 576), (64, 576), (64, 576), (256, 64), (256, 64), (256, 64), (256, 64))
Res2Fx = collections.namedtuple("Res2Fx", "x ws bs")


# ---------------------------------------------------------------- the restatements
def split_bias(b):
    """res2_chain_pack_kernel's bias fragment: (hi, lo) = (bf16(b), bf16(b - hi)) of the fp32 value, as float32 tensors."""
    b = b.float()
    hi = b.to(torch.bfloat16).float()
    return hi, (b - hi).to(torch.bfloat16).float()


def kernel_biases(bs, form):
    """The ten bias vectors a kernel form adds, as float64: conv1 x 4, conv2 x 3, conv3 x 3 with block 0's = fp32(b3 + bd).  form 0: the fp32
    values; form 1: hi + lo of their bf16 split."""
    b = [t.float() for t in bs]
    b = b[:7] + [b[7] + b[10], b[8], b[9]]
    if form == 1:
        return [sum(h.double() for h in split_bias(t)) for t in b]
    return [t.double() for t in b]


def res2(x, ws, bs, form=0, dtype=torch.float64, parts=False):
    """(y2, t1out), both unrounded, with every product, sum and bias in `dtype`.  parts=True also returns per block bneck_ref.block's parts
    and the rounded y, and for t1out its value before the ReLU and its sum of |terms|."""
    e = kernel_biases(bs, form)
    zero = torch.zeros(256, dtype=torch.float64)
    h, blocks, pre = x, [], None
    for k in range(3):
        ds = (ws[10], zero) if k == 0 else ()
        pre, p = BR.block(h, ws[k], e[k], ws[4 + k], e[4 + k], ws[7 + k], e[7 + k], *ds, dtype=dtype, parts=True)
        h = bf16_rne(pre)
        p["y"] = h
        blocks.append(p)
    w4, b4 = ws[3].to(dtype), e[3].to(dtype)
    a4 = h @ w4.t() + b4
    t1out = torch.relu(a4)
    if not parts:
        return pre, t1out
    return pre, t1out, {"blocks": blocks, "a4": a4, "mag4": h.abs() @ w4.abs().t() + b4.abs()}


def _patches7(roi):
    """[B,256,256,4] -> [B,128,128,196]: the 7 x 7 stride-2 pad-3 neighbourhoods, K = (ky*7 + kx)*4 + c."""
    B, H, W, C = roi.shape
    p = torch.zeros(B, H + 6, W + 6, C, dtype=roi.dtype)
    p[:, 3:-3, 3:-3] = roi
    return torch.cat([p[:, ky:ky + H:2, kx:kx + W:2] for ky in range(7) for kx in range(7)], dim=-1)


def _pool(c):
    """[B,128,128,C] -> [B,64,64,C]: 3 x 3 stride-2 pad-1 maximum; what lies outside the map takes no part (-inf)."""
    B, H, W, C = c.shape
    p = torch.full((B, H + 2, W + 2, C), float("-inf"), dtype=c.dtype)
    p[:, 1:-1, 1:-1] = c
    out = p[:, 0:H:2, 0:W:2]
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, p[:, dy:dy + H:2, dx:dx + W:2])
    return out


def stem(roi, w, bias, dtype=torch.float64, parts=False):
    """(pre, mag): the pooled map unrounded, and per output the largest sum of |terms| among the conv values of its pool window.  Frame by
    frame: the operand matrix of one frame is 25 MB in float64."""
    w, bias = w.to(dtype), bias.to(dtype)
    pre, mag, conv = [], [], []
    for b in range(roi.shape[0]):
        k = _patches7(roi[b:b + 1].to(dtype))
        a = k @ w.t() + bias
        pre.append(_pool(torch.relu(a)))
        mag.append(_pool(k.abs() @ w.abs().t() + bias.abs()))
        if parts:
            conv.append(a)
    pre, mag = torch.cat(pre), torch.cat(mag)
    return (pre, mag, torch.cat(conv)) if parts else (pre, mag)


def pack_stem(w):
    """[64, 196] -> the packed arena's filter bank [64][8 ky][8 px][4 ch] with ky == 7 and px == 7 zero (pack_stem_kernel's layout)."""
    out = torch.zeros(64, 8, 8, 4, dtype=w.dtype)
    out[:, :7, :7] = w.view(64, 7, 7, 4)
    return out


# ---------------------------------------------------------------- the cases
# kind -> (form of ivosw_res2_probe, tunables, the `ran` kind it must report); the probe library's defaults are put back after every case
DEFAULTS = {"R2C_PERSIST": 1, "R2C_GRID": 0}
KINDS = collections.OrderedDict((
    ("stage", (0, {}, 0)),                                   # res2_stage_kernel
    ("chain1", (1, {"R2C_PERSIST": 0}, 1)),                  # res2_chain_kernel<.., false>: one tile per workgroup
    ("chain5", (1, {"R2C_GRID": 5}, 2)),                     # persistent on 5 workgroups: 6 or 7 tiles each per frame
    ("chain", (1, {}, 2)),                                   # persistent, one workgroup per CU
))
CHAIN_KINDS = ("chain1", "chain5", "chain")
PHASES = 3
BIG = 0                         # frame count "one above CUs / 32": some workgroups of the default persistent grid own two tiles, some one
BIG_CPU = 9                     # ... what it is on the MI355X's 256 CUs, and what the CPU tests use
Case = collections.namedtuple("Case", "kind B y_s2 phase frac rev")


def frames(B, cus=256):
    return B if B != BIG else cus // 32 + 1


def _exact_cases():
    """Every kind meets every phase at both y forms; the frame counts 1, 2 and BIG rotate so that chain5 runs 2 frames, the default
    persistent grid BIG and every kind one.  The fractional-bias variant (phase 1) runs in descending tile order."""
    out = []
    for kind in KINDS:
        for phase in range(PHASES):
            for ys2 in (0, 1):
                out.append(Case(kind, (1, 2, BIG)[(phase + ys2) % 3], ys2, phase, False, 0))
        for ys2 in (0, 1):
            out.append(Case(kind, 1 + ys2, ys2, 1, True, 1))
    return tuple(out)


def _dense_cases():
    """phase: 0 = the plain recipe, 1 = every conv1 and conv2 bias strictly positive (the border case); frac unused."""
    out = []
    for kind in KINDS:
        out += [Case(kind, 1, 0, 0, False, 0), Case(kind, 2, 1, 0, False, 0), Case(kind, 2, 0, 1, False, 0)]
    return tuple(out)


EXACT_CASES, DENSE_CASES = _exact_cases(), _dense_cases()
MUST_REACH = frozenset(k + 4 * s for k in (0, 1, 2) for s in (0, 1))       # every *ran value ivosw_res2_probe can report
STEM_EXACT_FRAMES, STEM_DENSE_FRAMES = (1, 3, 9), (1, 3)                     # 9 frames: 576 tiles on 512 workgroups, the prefetch of a second tile


def case_id(c, dense=False):
    B = "big" if c.B == BIG else str(c.B)
    tail = ("-pos" if c.phase else "") if dense else f"-ph{c.phase}" + ("-frac" if c.frac else "")
    return f"{c.kind}-B{B}-s{c.y_s2}{tail}" + ("-rev" if c.rev else "")


def reported(c):
    return KINDS[c.kind][2] + 4 * c.y_s2


# ---------------------------------------------------------------- exact fixtures
def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_weights(phase, g):
    """Weights in {-1, 0, +1}: 2 nonzeros per 1x1 row, 3 taps (one per filter row) per 3x3 row, placed cyclically and rotated by `phase`.
    The 3x3 places are a bijection (row, phase, j) -> (tap, channel): the three phases put exactly one nonzero on each of its 576 K
    indices.  conv1 of blocks 1, 2 covers its 256 K indices with phases 0 and 1; every other layer in every phase."""
    p = phase

    def w3x3(i):
        def cols(r):
            taps = [3 * j + (p + j + i) % 3 for j in range(3)]
            return [t * 64 + (3 * r + 11 * t + 1 + 5 * i) % 64 for t in taps]
        return _sparse(64, 576, cols, g)
    w1_0 = _sparse(64, 64, lambda r: [(5 * r + 32 * j + p) % 64 for j in range(2)], g)
    w1_12 = [_sparse(64, 256, lambda r, i=i: [64 * q + (5 * r + 7 * q + p + 3 * i) % 64 for q in ((2 * p + j) % 4 for j in range(2))], g) for i in (1, 2)]
    w1_3 = _sparse(128, 256, lambda r: [64 * q + (5 * r + 7 * q + p) % 64 for q in ((2 * (r // 64) + j + 2 * p) % 4 for j in range(2))], g)
    w3 = [_sparse(256, 64, lambda r, i=i: [(3 * r + (32 + r // 64) * j + p + 9 * i) % 64 for j in range(2)], g) for i in range(3)]
    wd = _sparse(256, 64, lambda r: [(7 * r + (32 + r // 64) * j + 2 * p + 1) % 64 for j in range(2)], g)
    return (w1_0, w1_12[0], w1_12[1], w1_3, w3x3(0), w3x3(1), w3x3(2), w3[0], w3[1], w3[2], wd)


@functools.lru_cache(maxsize=None)
def exact_fixture(B, phase, frac=False):
    """Small integers throughout, so that no summation order can change a bit (test_res2_ref.py checks the conditions on ref64's own
    intermediates): x in [-2,2], random per element; the weights of exact_weights(phase); bneck_ref's integer bias ranges.  frac: every
    bias is n + 2^-10 - no bf16 value, but exact as hi + lo, and all sums stay multiples of 2^-10 below 2^14: exact in fp32."""
    g = torch.Generator().manual_seed(4000 + 10 * phase + frac)
    ws = exact_weights(phase, g)
    rng = (2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 2)                        # conv1: [-2,2], conv2: [-3,3], conv3: [-4,4], downsample: [-2,2]
    bs = tuple(_ints((s[0],), -r, r, g) + (2.0 ** -10 if frac else 0.0) for s, r in zip(W_SHAPES, rng))
    gx = torch.Generator().manual_seed(4100 + 10 * phase + frac)   # (weights and biases do not depend on the frame count)
    x = _ints((B, 64, 64, 64), -2, 2, gx)
    return Res2Fx(x, ws, bs)


@functools.lru_cache(maxsize=None)
def exact_want(B, phase, frac, form):
    """(bf16_rne(y2), bf16_rne(t1out)) of the exact fixture as float32: what the kernel's outputs must equal bit for bit."""
    y, t = res2(*exact_fixture(B, phase, frac), form=form)
    return bf16_rne(y).float() + 0.0, bf16_rne(t).float() + 0.0


def stem_exact_weights(g):
    """[64, 196] in {-1, 0, +1}: 2 nonzeros per filter row ky (28 K indices each) and output row; 3 is coprime to 28, so every one of the
    196 K indices meets a nonzero."""
    return _sparse(64, 196, lambda r: [28 * j + (3 * r + 5 * j + 13 * h) % 28 for j in range(7) for h in range(2)], g)


@functools.lru_cache(maxsize=None)
def stem_exact_fixture(B):
    g = torch.Generator().manual_seed(4500)
    w, bias = stem_exact_weights(g), _ints((64,), -4, 4, g)
    return _ints((B, 256, 256, 4), -3, 3, torch.Generator().manual_seed(4501)), w, bias


@functools.lru_cache(maxsize=None)
def stem_exact_want(B):
    return bf16_rne(stem(*stem_exact_fixture(B))[0]).float() + 0.0


# ---------------------------------------------------------------- dense fixtures
def _r16(t):
    return t.to(torch.bfloat16).float()


def _act(shape, g):
    """A post-ReLU tensor: relu(randn) scaled per channel, bf16 values (layer_ref's recipe)."""
    return _r16(torch.relu(torch.randn(shape, generator=g)) * (1 + torch.arange(shape[-1]) % 7 * 0.25))


def _wd(rows, K, g):
    """bneck_ref.dense_fixture's weights: randn / sqrt(K), scaled per row so that a swapped row or channel is not statistically invisible."""
    return _r16(torch.randn(rows, K, generator=g) / K ** 0.5 * (1 + torch.arange(rows)[:, None] % 5 * 0.5))


DENSE_FRAMES = max(max(c.B for c in DENSE_CASES), -(-DENSE_T1 // (64 * 64 * 64)))       # >= 2^19 t1 values of block 0


@functools.lru_cache(maxsize=None)
def dense_fixture(pos=0):
    """bneck_ref.dense_fixture's recipe: channel-scaled activations (>= 0: x is the pooled stem output), randn / sqrt(K) weights scaled per
    row, 0.1 * randn biases NOT rounded to bf16 (the chain kernel's hi + lo split is part of what is measured).  pos: the biases of every
    conv1 and conv2 are strictly positive (0.5 + |0.1 randn|): a halo pixel outside the frame that took relu(bias) instead of the 3x3's zero
    padding would move every border output far outside the element bound.  DENSE_FRAMES frames."""
    g = torch.Generator().manual_seed(5000 + pos)
    x = _act((DENSE_FRAMES, 64, 64, 64), g)
    ws = tuple(_wd(r, k, g) for r, k in W_SHAPES)
    bs = tuple(0.1 * torch.randn(s[0], generator=g) for s in W_SHAPES)
    if pos:
        bs = tuple(0.5 + b.abs() if i < 7 else b for i, b in enumerate(bs))
    return Res2Fx(x, ws, bs)


@functools.lru_cache(maxsize=None)
def dense_refs(pos, form):
    """((y64, t64), (y32, t32), (d32 of y, d32 of t1out)) over the whole dense batch, computed once and shared by every case of the form."""
    fx = dense_fixture(pos)
    r64, r32 = res2(*fx, form=form), res2(*fx, form=form, dtype=torch.float32)
    return r64, r32, tuple(bounds(a, b)[0] for a, b in zip(r64, r32))


def dense_figures(y, t1out, c):
    """bneck_ref.figures for y and for t1out on the first B frames of the dense batch: per output (worst element error over
    2^-8 |ref64| + 4 d32, mean error, d32, m32), d32 over the whole batch, m32 over the case's frames.  y is [B,64,64,256], or with y_s2 the
    even pixels - then so are its references (d32 stays the full maps')."""
    r64, r32, d32 = dense_refs(c.phase, KINDS[c.kind][0])
    B, s = c.B, 2 if c.y_s2 else 1
    sub = lambda t, i: t[:B, ::s, ::s] if i == 0 else t[:B]
    return tuple(figures(got, sub(r64[i], i), d32[i], bounds(sub(r64[i], i), sub(r32[i], i))[1]) for i, got in enumerate((y, t1out)))


STEM_K = 196


@functools.lru_cache(maxsize=None)
def stem_dense_fixture():
    """The ROI tile as the sampler leaves it: three normalised colour channels (randn, scaled per channel) and the mask probability in
    [0, 1]; randn / sqrt(K) filters scaled per row, 0.1 * randn biases; bf16 operands.  max(STEM_DENSE_FRAMES) frames."""
    g = torch.Generator().manual_seed(5500)
    B = max(STEM_DENSE_FRAMES)
    roi = torch.randn(B, 256, 256, 4, generator=g) * torch.tensor([1.0, 1.25, 1.5, 1.0])
    roi[..., 3] = torch.rand(B, 256, 256, generator=g)
    return _r16(roi), _wd(64, STEM_K, g), 0.1 * torch.randn(64, generator=g)


@functools.lru_cache(maxsize=None)
def stem_dense_refs():
    fx = stem_dense_fixture()
    r64, mag = stem(*fx)
    return r64, mag, stem(*fx, dtype=torch.float32)[0]


def stem_figures(out, B):
    """layer_ref.layer_figures' rule on the first B frames: |out - ref64| <= 2^-8 max(|ref64|, |out|) + (K + 2) 2^-23 mag for every element,
    K = 196 and mag the largest sum of |terms| in the pool window (the fp32 sum of the winning position, whichever it is, in ANY order),
    and mean |out - ref64| <= 1.5 m32.  Returns (worst element error over its bound, mean error, m32)."""
    r64, mag, r32 = (t[:B] for t in stem_dense_refs())
    od = out.double()
    err = (od - r64).abs()
    bound = 2.0 ** -8 * torch.maximum(r64.abs(), od.abs()) + (STEM_K + 2) * 2.0 ** -23 * mag
    return float((err / bound).max()), float(err.mean()), bounds(r64, r32)[1]
