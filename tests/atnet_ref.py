"""Host reference of the ATNet epilogue (csrc/atnet_epilogue.hip) in numpy: the float64 sigmoid the kernel's fp32 one is measured
against, and - exactly, in fp32 - everything behind the sigmoid: the three-step blend and the label rule of include/ivosw.h.
tests/test_atnet_option.py pins these against a literal restatement with torch CPU ops; the GPU tests share them."""
import numpy as np

FLT_MIN = 2.0 ** -126
# the sigmoid's bar against float64: err_kernel <= SIG_MULT * err_torch + SIG_FLOOR (tests/test_gpu_atnet_epilogue.py says where the
# figures behind SIG_MULT are recorded)
SIG_MULT = 2.0
SIG_FLOOR = 2.0 ** -24


def sigmoid64(x):
    """1 / (1 + exp(-x)) in float64, evaluated on the side that cannot overflow."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def alpha_beta32(alpha):
    """What torch makes of the Python scalars alpha and (1 - alpha) against a float32 tensor: each rounded to float32, 1 - alpha
    formed in float64 first."""
    return np.float32(alpha), np.float32(1 - np.float64(alpha))


def blend32(s, old, alpha):
    """(alpha * s) + ((1 - alpha) * old) as three separately rounded float32 operations (no FMA)."""
    a32, b32 = alpha_beta32(alpha)
    s, old = np.asarray(s, dtype=np.float32), np.asarray(old, dtype=np.float32)
    m1 = (a32 * s).astype(np.float32)
    m2 = (b32 * old).astype(np.float32)
    return (m1 + m2).astype(np.float32)


def labels(p, th):
    """p [n_obj, ...] float32 -> uint16 labels [...]: o* = first index of the maximum over objects; o* + 1 if p[o*] > float32(th)
    (strictly), else 0."""
    p = np.asarray(p, dtype=np.float32)
    am = np.argmax(p, axis=0)                          # numpy: the first maximum
    best = np.take_along_axis(p, am[None], 0)[0]
    return np.where(best > np.float32(th), am + 1, 0).astype(np.uint16)


def crop(a, pads):
    """[..., PH, PW] -> the window [..., H, W] of pads = (hpad1, hpad2, wpad1, wpad2); hpad2, wpad2 > 0."""
    h1, h2, w1, w2 = pads
    return a[..., h1:a.shape[-2] - h2, w1:a.shape[-1] - w2]
