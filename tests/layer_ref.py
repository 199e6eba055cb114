"""One bf16 conv layer of the tower, and res3's first block behind its conv1 (csrc/stage_first.hip), restated in plain torch on the CPU,
with the fixtures, bounds and the case table that tests/test_gpu_layer_kernels.py holds the layer kernels to - conv_igemm_dma_kernel,
conv_igemm_ws_kernel, conv3x3_patch_kernel (csrc/conv.hip), conv1x1_wide_kernel (csrc/bottleneck_wide.hip), gemm_8phase_kernel
(csrc/gemm_8phase.h) and stage_first_kernel, each launched alone through ivosw_conv_probe / ivosw_stage_first_probe
(include/ivosw_probe.h).  tests/test_layer_ref.py pins this file on the CPU.  No GPU is needed for anything in it.

Layout (ConvArgs, csrc/conv.h): x [B,H,W,Cin] NHWC; w [Cout, ksize*ksize*Cin (+ Cin2)] with K = (ky*ksize + kx)*Cin + c and the columns of
the optional second pixel source x2 [B,H2,W2,Cin2] behind them; fp32 bias; optional residual res [B,Ho,Wo,Cout].  Operands are bf16 values, widened.

    pre = act(conv(x, w[:, :K1]; ksize, stride, pad) [+ x2 sampled at (oy*stride2, ox*stride2) @ w[:, K1:]^T] + bias [+ res])

and for stage_first (t1 [B,64,64,128], x2 [B,64,64,256] at stride2 2 or [B,32,32,256] at stride2 1, w2 [128, 9*128], wc [512, 128 + 256]):

    t2  = bf16_rne(relu(conv3x3 stride 2 pad 1 (t1, w2) + b2))
    pre = relu([t2 | x2 sampled] @ wc^T + bc)

`layer` and `stage_first` return pre UNROUNDED (the kernels' output is bf16_rne(pre)).  The rounding points are those of the kernels'
epilogues, read from the sources: a layer rounds ONCE.  The generic kernels (epilogue_store, and the patch kernel's own store pass) add
the bias and then the widened bf16 residual to the fp32 accumulator, in fp32, and pack the pair (act2_bf16: round to nearest even) with
the ReLU; conv1x1_wide_kernel and gemm_8phase_kernel start the accumulator from the bias, add the widened residual in fp32 and pack in
the same way.  Whether the ReLU comes before or after the pack gives the same bits: rounding is monotonic and keeps the sign.
stage_first_kernel rounds t2 on its way into LDS (relu2_bf16 after the fp32 bias) and the output once (bias as the initial accumulator).
No kernel rounds anywhere else, so nothing here deviates from the lines above.
"""
import collections
import functools

import torch

from tests.bneck_ref import DENSE_T1, NAN_BITS, _sparse, _taps, bf16_rne, bounds, figures  # noqa: F401  (re-exported for the tests)


# ---------------------------------------------------------------- the restatements
def _gather(x, ksize, stride, pad):
    """[B,H,W,C] -> [B,Ho,Wo,ksize*ksize*C]: the operand rows of the layer as a matrix, K = (ky*ksize + kx)*C + c."""
    if ksize == 1:
        assert pad == 0
        return x[:, ::stride, ::stride]
    assert ksize == 3 and pad == 1
    if stride == 1:
        return _taps(x)
    B, H, W, C = x.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x
    return torch.cat([p[:, ky:ky + H:stride, kx:kx + W:stride] for ky in range(3) for kx in range(3)], dim=-1)


def operand_rows(x, ksize=1, stride=1, pad=0, x2=None, stride2=1):
    k = _gather(x, ksize, stride, pad)
    if x2 is not None:
        assert ksize == 1
        Ho, Wo = k.shape[1:3]
        k = torch.cat([k, x2[:, ::stride2, ::stride2][:, :Ho, :Wo]], dim=-1)
    return k


def layer(x, w, bias, ksize=1, stride=1, pad=0, relu=True, res=None, x2=None, stride2=1, dtype=torch.float64):
    """(pre, mag): the layer above with every product, sum, bias and residual in `dtype`, unrounded, and per output element the sum of the
    magnitudes of every term (products, bias, residual): what a summation error is proportional to."""
    c = lambda t: None if t is None else t.to(dtype)
    x, w, bias, res, x2 = map(c, (x, w, bias, res, x2))
    k = operand_rows(x, ksize, stride, pad, x2, stride2)
    assert k.shape[-1] == w.shape[1], (k.shape, w.shape)
    pre = k @ w.t() + bias
    mag = k.abs() @ w.abs().t() + bias.abs()
    if res is not None:
        pre, mag = pre + res, mag + res.abs()
    return (torch.relu(pre) if relu else pre), mag


def stage_first(t1, x2, w2, b2, wc, bc, stride2, dtype=torch.float64, parts=False):
    c = lambda t: t.to(dtype)
    t1, x2, w2, b2, wc, bc = map(c, (t1, x2, w2, b2, wc, bc))
    k2 = _gather(t1, 3, 2, 1)
    a2 = k2 @ w2.t() + b2
    t2 = bf16_rne(torch.relu(a2))
    k3 = torch.cat([t2, x2[:, ::stride2, ::stride2]], dim=-1)
    pre = torch.relu(k3 @ wc.t() + bc)
    if not parts:
        return pre
    return pre, {"a2": a2, "t2": t2, "mag": (k2.abs() @ w2.abs().t() + b2.abs(), k3.abs() @ wc.abs().t() + bc.abs())}


# ---------------------------------------------------------------- the instantiations and the selector, restated
# enum ConvKernel of csrc/conv.h, in its order (test_layer_ref.py reads the header and compares)
CONV_KERNELS = ("CK_STEM", "CK_PATCH_2F", "CK_PATCH_4F_KXY", "CK_PATCH_4F", "CK_PATCH_KXY", "CK_PATCH", "CK_DMA_SMALL", "CK_WS_LW8", "CK_WS_LW4",
                "CK_DMA", "CK_DMA_SHORTK", "CK_PATCH_X3", "CK_WS64", "CK_DMA64", "CK_DMA64_SHORTK")
BF16_SELECTOR_IDS = tuple(k for k in CONV_KERNELS if k not in ("CK_STEM", "CK_PATCH_X3"))     # what a bf16 layer can reach
# the tunables the cases move, with the defaults the sources read them with: every case sets its own and puts these back
DEFAULTS = {"SMALL_GRID": 128, "LW": 8, "WS": 1, "NK": 8, "PATCH3": 1, "PATCH_KEYXY": 0, "PATCH_SMALL": 128, "WIDE_SMALL": 0}

# path: "sel" = kernel 0 of ivosw_conv_probe (conv_select), "wide" = 1, "g8" = 2, "sf" = ivosw_stage_first_probe
# x2: None or (H2, Cin2, stride2); reaches: a ConvKernel name | "NPT8" / "NPT4" | "RES0" / "RES1" | "SF"
Layer = collections.namedtuple("Layer", "name H Cin Cout ksize stride pad res x2")
Case = collections.namedtuple("Case", "layer path frames tune reaches")


def _L(name, H, Cin, Cout, ksize=1, stride=1, res=False, x2=None):
    return Layer(name, H, Cin, Cout, ksize, stride, 1 if ksize == 3 else 0, res, x2)


LAYERS = {l.name: l for l in (
    _L("s2_128", 64, 128, 128, 3, 2), _L("s2_256", 32, 256, 256, 3, 2), _L("s2_512", 16, 512, 512, 3, 2),       # the stride-2 3x3 of res3 / res4 / res5
    _L("red5", 8, 2048, 512),                                                                                   # res5's identity-block conv1
    _L("p512", 8, 512, 512, 3), _L("p256", 16, 256, 256, 3), _L("p128", 32, 128, 128, 3),                        # stride-1 3x3: the patch kernel's shapes
    _L("exp2", 64, 64, 256, res=True), _L("exp3", 32, 128, 512, res=True),                                      # conv3 + residual, K <= 128
    _L("c64", 64, 64, 64), _L("red2", 64, 256, 64), _L("t64", 64, 64, 64, 3),                                   # Cout == 64: res2's layers
    _L("cat2", 64, 64, 256, x2=(64, 64, 1)), _L("cat3", 32, 128, 512, x2=(64, 256, 2)),                         # [conv3 | downsample], K-extension
    _L("exp5", 8, 512, 2048, res=True),                                                                         # res5's conv3 + residual
    _L("red4", 32, 512, 256), _L("red5a", 16, 1024, 512),                                                       # first-block reductions of res4 / res5
    _L("cat4", 16, 256, 1024, x2=(32, 512, 2)), _L("cat5", 8, 512, 2048, x2=(16, 1024, 2)),
)}
SF_ARMS = {"sf_s2": (64, 2), "sf_s1": (32, 1)}      # stage_first: (H2 = W2, stride2)


def _cases():
    out = []
    add = lambda names, path, frames, tune, reaches: out.extend(Case(n, path, frames, tune, reaches) for n in names.split())
    SG0 = {"SMALL_GRID": 0}
    add("s2_128", "sel", (1, 3), {}, "CK_DMA_SMALL")
    add("s2_128", "sel", (1, 3), SG0, "CK_WS_LW8")
    add("s2_128", "sel", (1, 3), {**SG0, "LW": 4}, "CK_WS_LW4")
    add("s2_128", "sel", (1, 3), {**SG0, "WS": 0}, "CK_DMA")
    add("s2_256 s2_512 red5", "sel", (1, 3, 5), {}, "CK_DMA_SMALL")
    add("s2_256 s2_512 red5", "sel", (1, 3, 5), SG0, "CK_WS_LW8")
    add("p512", "sel", (1, 3, 4, 5), {}, "CK_PATCH_2F")
    add("p512", "sel", (1, 3, 4, 5), {"PATCH_SMALL": 0}, "CK_PATCH_4F")
    add("p512", "sel", (1, 3, 4, 5), {"PATCH_KEYXY": 1}, "CK_PATCH_4F_KXY")
    add("p256 p128", "sel", (1, 3), {}, "CK_PATCH")
    add("p256 p128", "sel", (1, 3), {"PATCH_KEYXY": 1}, "CK_PATCH_KXY")
    add("p256 p128", "sel", (1, 3), {"PATCH3": 0}, "CK_DMA_SMALL")                  # the per-tap arm
    add("exp2 exp3", "sel", (1, 2), {}, "CK_DMA_SHORTK")
    add("c64", "sel", (1, 2), {}, "CK_DMA64_SHORTK")
    add("red2 t64", "sel", (1, 2), {}, "CK_WS64")
    add("red2 t64", "sel", (1, 2), {"WS": 0}, "CK_DMA64")
    add("cat2 cat3", "sel", (1, 3), {}, "CK_DMA_SHORTK")                             # K = 128 / 384: not above NK = 8 K-tiles
    add("cat3", "sel", (1, 3), {"NK": 4, **SG0}, "CK_WS_LW8")                        # ... and the K-extension through the loader waves
    add("cat3", "sel", (1, 3), {"NK": 4}, "CK_DMA_SMALL")
    # K = 512 is 8 K-tiles, not above NK = 8: the default is the 128 x 128 tile; NK = 4 takes the layer to the 256 x 128 tiles
    add("exp5", "sel", (3,), {}, "CK_DMA_SHORTK")
    add("exp5", "sel", (3,), {"NK": 4, **SG0}, "CK_WS_LW8")
    add("exp5", "sel", (3,), {"NK": 4, **SG0, "WS": 0}, "CK_DMA")
    add("red4 red5a cat4 cat5 exp5", "wide", (1, 3, 5), {}, "NPT8")
    add("red4 red5a cat4 cat5 exp5", "wide", (1, 3, 5), {"WIDE_SMALL": 1 << 20}, "NPT4")
    add("red4 red5a cat4 cat5", "g8", (1, 3, 5), {}, "RES0")
    add("exp5", "g8", (1, 3, 5), {}, "RES1")
    add("sf_s2 sf_s1", "sf", (1, 3), {}, "SF")
    return tuple(out)


CASES = _cases()
# what the table must reach: every bf16 id of the selector, both NPT forms of the wide kernel, both RES forms of the 8-phase kernel
MUST_REACH = frozenset(BF16_SELECTOR_IDS) | {"NPT8", "NPT4", "RES0", "RES1", "SF"}


def case_id(c, B):
    return f"{c.layer}-{c.path}-B{B}-{c.reaches}" + "".join(f"-{k}{v}" for k, v in sorted(c.tune.items()))


def case_params():
    """(case, B) for every row and frame count, with ids."""
    return [(c, B) for c in CASES for B in c.frames]


def out_hw(l):
    return (l.H + 2 * l.pad - l.ksize) // l.stride + 1


def k_total(l):
    return l.ksize * l.ksize * l.Cin + (l.x2[1] if l.x2 else 0)


def select(l, B, tune):
    """conv_select (csrc/conv.hip) for a bf16 layer, restated: the id a selector case must report."""
    t = {**DEFAULTS, **tune}
    Ho = out_hw(l)
    M, nk = B * Ho * Ho, k_total(l) // 64
    if l.Cout % 128 == 0:
        grid = -(-M // 256) * (l.Cout // 128)
        patch_ok = l.ksize == 3 and l.stride == 1 and l.pad == 1 and not l.res and l.Cin % 64 == 0 and l.H in (32, 16, 8)
        if patch_ok and t["PATCH3"]:
            kxy = t["PATCH_KEYXY"] != 0
            if l.H == 8 and not kxy and grid < t["PATCH_SMALL"]:
                return "CK_PATCH_2F"
            if l.H == 8:
                return "CK_PATCH_4F_KXY" if kxy else "CK_PATCH_4F"
            return "CK_PATCH_KXY" if kxy else "CK_PATCH"
        deep = nk > t["NK"]
        if deep and grid < t["SMALL_GRID"]:
            return "CK_DMA_SMALL"
        if deep and t["WS"]:
            return "CK_WS_LW8" if t["LW"] == 8 else "CK_WS_LW4"
        return "CK_DMA" if deep else "CK_DMA_SHORTK"
    if nk >= 4 and t["WS"]:
        return "CK_WS64"
    return "CK_DMA64" if nk >= 2 else "CK_DMA64_SHORTK"


def expected(c, B):
    """The instantiation a case must reach by the sources' own rules (test_layer_ref.py holds the table's `reaches` to this)."""
    if c.path == "sf":
        return "SF"
    l = LAYERS[c.layer]
    if c.path == "sel":
        return select(l, B, c.tune)
    if c.path == "wide":
        Ho = out_hw(l)
        return "NPT4" if -(-B * Ho * Ho // 256) * (l.Cout // 256) < {**DEFAULTS, **c.tune}["WIDE_SMALL"] else "NPT8"
    return "RES1" if l.res else "RES0"


def reported(c, ran):
    """The name of what a probe call reported through its `ran`."""
    return CONV_KERNELS[ran] if c.path == "sel" else (f"NPT{ran}" if c.path == "wide" else f"RES{ran}")


# ---------------------------------------------------------------- fixtures
def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _ints(shape, g):
    """bneck_ref.exact_fixture's activations: [-3,3] on even and [-1,2] on odd channels, random per element."""
    x = torch.randint(-3, 4, shape, generator=g).float()
    x[..., 1::2] = torch.randint(-1, 3, shape[:-1] + (shape[-1] // 2,), generator=g).float()
    return x


def _w3x3(C, g):
    """[C, 9*C]: one nonzero per tap and row, every K index met (3 is coprime to C)."""
    return _sparse(C, 9 * C, lambda r: [j * C + (3 * r + 11 * j + 1) % C for j in range(9)], g)


def _w1x1(rows, K, g):
    """[rows, K], 8 nonzeros per row an eighth of K apart; the first K / 8 rows meet every K index, the others shift theirs."""
    s = K // 8
    assert rows >= s
    return _sparse(rows, K, lambda r: [(r + j * s + 7 * j * ((r // s) % 5)) % K for j in range(8)], g)


@functools.lru_cache(maxsize=None)
def exact_fixture(name, B):
    """Small integers throughout, so that no summation order can change a bit (test_layer_ref.py checks the conditions on ref64's own
    intermediates).  A layer: dict x, w, bias, res, x2 (None where the layer has none); stage_first: (t1, x2, w2, b2, wc, bc)."""
    g = torch.Generator().manual_seed(100 * _seed(name) + B)
    if name in SF_ARMS:
        H2 = SF_ARMS[name][0]
        return (_ints((B, 64, 64, 128), g), _ints((B, H2, H2, 256), g), _w3x3(128, g), torch.randint(-3, 4, (128,), generator=g).float(),
                _w1x1(512, 384, g), torch.randint(-4, 5, (512,), generator=g).float())
    l = LAYERS[name]
    Ho = out_hw(l)
    fx = {"x": _ints((B, l.H, l.H, l.Cin), g), "res": None, "x2": None}
    if l.ksize == 3:
        assert l.Cin == l.Cout
        fx["w"] = _w3x3(l.Cin, g)
    else:
        fx["w"] = _w1x1(l.Cout, k_total(l), g)
    fx["bias"] = torch.randint(-4, 5, (l.Cout,), generator=g).float()
    if l.res:
        fx["res"] = _ints((B, Ho, Ho, l.Cout), g)
    if l.x2:
        fx["x2"] = _ints((B, l.x2[0], l.x2[0], l.x2[1]), g)
    return fx


def _r16(t):
    return t.to(torch.bfloat16).float()


def _act(shape, g):
    """A post-ReLU tensor: relu(randn) scaled per channel (as tests/test_gpu_res4_chain_sched.py draws its x), bf16 values."""
    return _r16(torch.relu(torch.randn(shape, generator=g)) * (1 + torch.arange(shape[-1]) % 7 * 0.25))


def _wd(rows, K, g):
    """bneck_ref.dense_fixture's weights: randn / sqrt(K), scaled per row so that a swapped row or channel is not statistically invisible."""
    return _r16(torch.randn(rows, K, generator=g) / K ** 0.5 * (1 + torch.arange(rows)[:, None] % 5 * 0.5))


def max_frames(name):
    return max(B for c in CASES if c.layer == name for B in c.frames)


# d32 is taken over 2^20 t2 values, twice bneck_ref.DENSE_T1: what a flipped t2 costs spreads over two orders of magnitude with the channel
# and row scales of the recipe, and a fp32 reordering flips about 7 values per frame (test_layer_ref.py prints them)
SF_DENSE_FRAMES = max(3, -(-2 * DENSE_T1 // (32 * 32 * 128)))


@functools.lru_cache(maxsize=None)
def dense_fixture(name):
    """The probe tools' recipe (randn / sqrt(K) weights, 0.1 * randn biases, bf16 values) with bneck_ref.dense_fixture's per-channel scaling;
    x, x2, res, t1 stand for post-ReLU tensors and are >= 0.  Holds max_frames(name) frames (stage_first: SF_DENSE_FRAMES); a case of B
    frames runs on the first B (frames are independent of each other in every kernel)."""
    g = torch.Generator().manual_seed(7000 + _seed(name))
    if name in SF_ARMS:
        H2, B = SF_ARMS[name][0], SF_DENSE_FRAMES
        return (_act((B, 64, 64, 128), g), _act((B, H2, H2, 256), g), _wd(128, 1152, g), 0.1 * torch.randn(128, generator=g),
                _wd(512, 384, g), 0.1 * torch.randn(512, generator=g))
    l, B = LAYERS[name], max_frames(name)
    Ho = out_hw(l)
    fx = {"x": _act((B, l.H, l.H, l.Cin), g), "w": _wd(l.Cout, k_total(l), g), "bias": 0.1 * torch.randn(l.Cout, generator=g), "res": None, "x2": None}
    if l.res:
        fx["res"] = _act((B, Ho, Ho, l.Cout), g)
    if l.x2:
        fx["x2"] = _act((B, l.x2[0], l.x2[0], l.x2[1]), g)
    return fx


def first_frames(fx, B):
    """The operands of a kernel case: the first B frames of a fixture."""
    if isinstance(fx, dict):
        return {k: (v[:B].contiguous() if k in ("x", "res", "x2") and v is not None else v) for k, v in fx.items()}
    return (fx[0][:B].contiguous(), fx[1][:B].contiguous()) + fx[2:]


def layer_ref(name, fx, dtype=torch.float64):
    l = LAYERS[name]
    return layer(fx["x"], fx["w"], fx["bias"], l.ksize, l.stride, l.pad, True, fx["res"], fx["x2"], l.x2[2] if l.x2 else 1, dtype)


def sf_ref(name, fx, dtype=torch.float64, parts=False):
    return stage_first(*fx, stride2=SF_ARMS[name][1], dtype=dtype, parts=parts)


@functools.lru_cache(maxsize=None)
def exact_want(name, B):
    """bf16_rne(ref64) of the exact fixture as float32: what the kernel's output must equal bit for bit."""
    fx = exact_fixture(name, B)
    return bf16_rne(sf_ref(name, fx) if name in SF_ARMS else layer_ref(name, fx)[0]).float() + 0.0


@functools.lru_cache(maxsize=None)
def dense_refs(name):
    """Over the whole dense batch, computed once and shared by every frame count and arm.  A layer: (ref64, mag, ref32);
    stage_first: (ref64, ref32, d32)."""
    fx = dense_fixture(name)
    if name in SF_ARMS:
        r64, r32 = sf_ref(name, fx), sf_ref(name, fx, torch.float32)
        return r64, r32, bounds(r64, r32)[0]
    r64, mag = layer_ref(name, fx)
    return r64, mag, layer_ref(name, fx, torch.float32)[0]


def layer_figures(y, name, B):
    """A single layer's two figures on the first B frames of its dense batch, from the references alone:
        |y - ref64| <= 2^-8 max(|ref64|, |y|) + (K + 2) 2^-23 mag      for every element
    (the output's own bf16 rounding + the worst case of an fp32 sum of K products, a bias and a residual in ANY order, at unit roundoff 2^-23,
    which also covers an accumulator that truncates), and mean |y - ref64| <= 1.5 m32 with m32 = mean |bf16_rne(ref32) - ref64|.
    Returns (worst element error over its bound, mean error, m32)."""
    r64, mag, r32 = (t[:B] for t in dense_refs(name))
    yd = y.double()
    err = (yd - r64).abs()
    bound = 2.0 ** -8 * torch.maximum(r64.abs(), yd.abs()) + (k_total(LAYERS[name]) + 2) * 2.0 ** -23 * mag
    return float((err / bound).max()), float(err.mean()), bounds(r64, r32)[1]


def sf_figures(y, name, B):
    """stage_first has t2's intermediate rounding: the bottleneck kernels' rule unchanged (bneck_ref.figures), d32 over the whole dense batch."""
    r64, r32, d32 = dense_refs(name)
    return figures(y, r64[:B], d32, bounds(r64[:B], r32[:B])[1])
