"""TEST INFRASTRUCTURE (never imported by the product path): a float64 reference of the segmentation epilogue
(csrc/seg_epilogue.hip: bilinear upsampling with align_corners, argmax, softmax), the error bound of its float32
evaluation, and the inputs the CPU and GPU tests share.

Two stages.

1. *The operation's definition* (ATen ``upsample_bilinear2d``, ``align_corners=True``), in float32 because ATen defines
   it there: ``scale = float32(in - 1) / float32(out - 1)`` (0 when out == 1), ``src = scale * float32(dst)`` (one
   float32 product), ``i0 = trunc(src)``, ``i1 = i0 + (i0 < in - 1)``, ``lambda = src - i0`` (exact in float32: a
   difference of a float and its own integer part).  A different ``src`` would be a different operation, not a rounding
   error, so these steps are reproduced bit for bit (``coords``).

2. *Everything after that in float64*: ``1 - lambda``, the two horizontal lerps, the vertical lerp, the maximum,
   ``exp(x - max)``, the sum and the division (``Ref``).

The bound.  ``sample()`` in the kernel (and ATen's CPU kernel) evaluates, with u = 2^-24 and every operation rounded once,

    w0 = fl(1 - lw)                          (1 + d1)
    top = fl(fl(w0 * a) + fl(lw * b))        (1 + d2), (1 + d3), then (1 + d4)
    bot likewise
    out = fl(fl(h0 * top) + fl(lh * bot))    h0 = fl(1 - lh): (1 + d5); products (1 + d6), (1 + d7); sum (1 + d8)

The tap ``a`` reaches the result through w0 (d1), its product (d2), the horizontal sum (d4), h0 (d5), the vertical product
(d6) and the vertical sum (d8): six roundings, the longest chain (``b`` and the ``bot`` taps skip d1 and / or d5).  With
non-negative weights that sum to one and M = max |tap|, the exact result is a convex combination of the taps and

    |out - exact| <= ((1 + u)^6 - 1) * M  <  6.000004 u M  <=  K u M        with K = 7

(K = 6 is the first-order count; 7 absorbs the higher-order terms and a fused multiply-add on either side, which only
removes roundings).  ``BOUND_K = 7``: the upsampled logits of any faithful float32 evaluation lie within
``7 * 2^-24 * M`` of stage 2, M taken over the four taps of that pixel and channel.

Labels.  Two classes can change places only when both errors together reach their gap: at a pixel whose float64 top-two
gap exceeds ``2 * 7 u * max_c M_c`` the label must be the float64 argmax; elsewhere either of the two best is accepted,
and such pixels may make up at most ``NEAR_TIE_CAP = 1e-3`` of a case (asserted on the reference alone, CPU test).
"""
import collections

import numpy as np
import torch

BOUND_K = 7
U = 2.0 ** -24
NEAR_TIE_CAP = 1e-3
FLT_MIN = 2.0 ** -126


def coords(n_in, n_out):
    """-> (i0 int64 [n_out], step int64 [n_out] in {0, 1}, lam float32 [n_out]): ATen's source index and weight, bit for bit."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = src.astype(np.int64)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, (i0 < n_in - 1).astype(np.int64), lam


def _taps(x, H, W):
    hs, ws = x.shape[-2:]
    y0, ys, ly = coords(hs, H)
    x0, xs, lx = coords(ws, W)
    r0, r1 = x[..., y0, :], x[..., y0 + ys, :]
    return (r0[..., x0], r0[..., x0 + xs], r1[..., x0], r1[..., x0 + xs]), ly, lx


def upsample64(x, H, W):
    """float32 logits [k,C,hs,ws] -> (float64 upsampled [k,C,H,W], M = largest |tap| per value)."""
    x = np.asarray(x, np.float32)
    (a, b, c, d), ly, lx = _taps(x.astype(np.float64), H, W)
    ly, lx = ly.astype(np.float64)[:, None], lx.astype(np.float64)[None, :]
    top = (1.0 - lx) * a + lx * b
    bot = (1.0 - lx) * c + lx * d
    M = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))
    return (1.0 - ly) * top + ly * bot, M


def upsample_f32_model(x, H, W):
    """The kernel's ``sample()`` operation by operation in numpy float32 (no fused multiply-add): a faithful float32 evaluation
    to try the bound on where there is no GPU."""
    x = np.asarray(x, np.float32)
    (a, b, c, d), ly, lx = _taps(x, H, W)
    ly, lx = ly[:, None], lx[None, :]
    one = np.float32(1.0)
    w0, h0 = one - lx, one - ly
    top = w0 * a + lx * b
    bot = w0 * c + lx * d
    out = h0 * top + ly * bot
    assert out.dtype == np.float32
    return out


Ref = collections.namedtuple("Ref", "up bound label second gap near_tie probs")


def reference(x, H, W):
    """Everything the tests compare against, from float32 logits [k,C,hs,ws]:
    up float64 [k,C,H,W]; bound [k,C,H,W] = K u M; label = float64 argmax (first maximum) and second = the runner-up [k,H,W]; gap of
    the two; near_tie = gap <= 2 K u max_c M; probs = float64 softmax."""
    up, M = upsample64(x, H, W)
    bound = BOUND_K * U * M
    C = up.shape[1]
    order = np.argsort(-up, axis=1, kind="stable")
    label = order[:, 0]
    second = order[:, 1] if C > 1 else order[:, 0]
    top = np.take_along_axis(up, label[:, None], 1)[:, 0]
    gap = top - np.take_along_axis(up, second[:, None], 1)[:, 0] if C > 1 else np.full(top.shape, np.inf)
    near = gap <= 2.0 * bound.max(axis=1)
    e = np.exp(up - top[:, None])
    return Ref(up, bound, label, second, gap, near, e / e.sum(axis=1, keepdims=True))


def check_labels(got, ref):
    """got [k,H,W] integer labels: the float64 argmax at every clear pixel, one of the two best at a near-tie.  -> number of flips."""
    got = np.asarray(got).astype(np.int64)
    clear = ~ref.near_tie
    wrong = clear & (got != ref.label)
    assert not wrong.any(), f"{int(wrong.sum())} labels differ from the float64 argmax at clear pixels, first at {np.argwhere(wrong)[0].tolist()}"
    tie_ok = (got == ref.label) | (got == ref.second)
    assert tie_ok[ref.near_tie].all(), "a near-tie pixel carries a class that is neither of the two best"
    assert ref.near_tie.mean() <= NEAR_TIE_CAP
    return int((got != ref.label).sum())


def torch_fp32(x, H, W):
    """(upsampled logits, softmax) of torch's float32 CPU kernels, the reference's own calls."""
    up = torch.nn.functional.interpolate(torch.from_numpy(np.asarray(x, np.float32)), size=(H, W), mode="bilinear", align_corners=True)
    return up.numpy(), torch.softmax(up, 1).numpy()


# ------------------------------------------------------------------------------------------------ inputs
def logits(k, C, hs, ws, seed, variant="plain"):
    """Smooth blobs + fine noise (the generator of tests/test_gpu_seg_epilogue.py), float32 numpy [k,C,hs,ws].
    variant: plain | offset (+ 100: large |logit|, small differences) | wide (x 20: a channel spread of about +-60, exp(x - max)
    underflows float32 for the losing channels)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(k, C, max(2, hs // 6), max(2, ws // 6), generator=g) * 3.0
    x = torch.nn.functional.interpolate(base, size=(hs, ws), mode="bicubic", align_corners=False)
    x = (x + 0.3 * torch.randn(k, C, hs, ws, generator=g)).contiguous()
    if variant == "offset":
        x = x + 100.0
    elif variant == "wide":
        x = x * 20.0
    else:
        assert variant == "plain"
    return x.numpy().astype(np.float32)


SegCase = collections.namedtuple("SegCase", "name k C hs ws H W variant kernel")

# kernel = the instantiation the launcher picks for the aligned all-outputs call: "<CMAX,V,FULL>" or "generic"
CASES = [SegCase(*c) for c in [
    # every register instantiation; V = 4 threads straddle a row end where W % 4 != 0
    ("full4", 2, 4, 9, 11, 12, 13, "plain", "<4,4,full>"),
    ("full4_offset", 2, 4, 9, 11, 12, 13, "offset", "<4,4,full>"),
    ("full4_wide", 2, 4, 9, 11, 12, 13, "wide", "<4,4,full>"),
    ("full8", 1, 8, 5, 6, 4, 7, "plain", "<8,4,full>"),
    ("full8_wide", 1, 8, 5, 6, 24, 30, "wide", "<8,4,full>"),
    ("full16", 1, 16, 7, 9, 20, 31, "plain", "<16,4,full>"),
    ("c3_v4", 1, 3, 10, 12, 24, 30, "plain", "<4,4>"),
    ("c5_v4", 2, 5, 8, 8, 16, 18, "plain", "<8,4>"),
    ("c11_v4", 1, 11, 6, 7, 12, 13, "plain", "<16,4>"),
    ("c11_v4_offset", 1, 11, 6, 7, 12, 13, "offset", "<16,4>"),
    ("c3_v1", 1, 3, 5, 5, 9, 9, "plain", "<4,1>"),
    ("c6_v1", 2, 6, 7, 5, 15, 13, "plain", "<8,1>"),
    ("c6_v1_offset", 2, 6, 7, 5, 15, 13, "offset", "<8,1>"),
    ("c13_v1", 1, 13, 4, 6, 11, 9, "plain", "<16,1>"),
    ("c13_v1_wide", 1, 13, 4, 6, 11, 9, "wide", "<16,1>"),
    ("c17", 1, 17, 6, 6, 13, 14, "plain", "generic"),
    ("c17_offset", 1, 17, 6, 6, 13, 14, "offset", "generic"),
    ("c20", 1, 20, 5, 7, 16, 10, "plain", "generic"),
    ("c20_wide", 1, 20, 5, 7, 16, 10, "wide", "generic"),
    # geometry
    ("down_both", 1, 4, 40, 50, 13, 16, "plain", "<4,4,full>"),
    ("down_h_up_w", 1, 4, 40, 6, 10, 24, "plain", "<4,4,full>"),
    ("up_h_down_w", 1, 3, 5, 60, 21, 20, "plain", "<4,4>"),
    ("row_target", 1, 4, 3, 9, 1, 36, "plain", "<4,4,full>"),
    ("column_target", 1, 4, 9, 3, 36, 1, "plain", "<4,4,full>"),
    ("row_source", 1, 4, 1, 9, 8, 30, "plain", "<4,4,full>"),
    ("column_source", 1, 5, 9, 1, 9, 7, "plain", "<8,1>"),
    ("identity4", 2, 4, 12, 10, 12, 10, "plain", "<4,4,full>"),
    ("identity4_wide", 2, 4, 12, 10, 12, 10, "wide", "<4,4,full>"),
    ("identity4_offset", 2, 4, 12, 10, 12, 10, "offset", "<4,4,full>"),
    ("identity20", 1, 20, 12, 10, 12, 10, "plain", "generic"),
    ("identity20_wide", 1, 20, 12, 10, 12, 10, "wide", "generic"),
    ("long_row", 1, 4, 2, 300, 4, 1200, "plain", "<4,4,full>"),          # src up to 299: the coordinate's ulp is largest
    ("long_row_offset", 1, 4, 2, 300, 4, 1200, "offset", "<4,4,full>"),
]]


def expected_kernel(C, H, W):
    """The launcher's choice for 16-byte aligned, all-outputs calls with dense strides."""
    if C > 16:
        return "generic"
    cm = 4 if C <= 4 else 8 if C <= 8 else 16
    if (H * W) % 4:
        return f"<{cm},1>"
    return f"<{cm},4,full>" if C == cm else f"<{cm},4>"


def case_logits(c):
    return logits(c.k, c.C, c.hs, c.ws, seed=1000 + 7 * c.C + c.hs * c.ws, variant=c.variant)


def logits_256():
    """C = 256 at 3 x 4 -> 6 x 10, with source pixels where class 255 (and class 0, and class 128) wins by a wide margin."""
    x = logits(1, 256, 3, 4, seed=256)
    x[0, 255, 2, 3] += 40.0
    x[0, 255, 2, 2] += 40.0
    x[0, 128, 0, 0] += 40.0
    x[0, 0, 0, 3] += 40.0
    return x
