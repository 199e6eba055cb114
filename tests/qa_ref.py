"""A numpy / torch-CPU restatement of the assessment-sample path (csrc/qa.hip, the byte-plane count source and ivosw_qa_targets of
csrc/metrics.hip): the quantiser, the threshold, the per-unit targets in the assessment's unit order and the reference training loop's
loss / diff (quality_assessment.py:235-263).  Shared by tests/test_qa_option.py (CPU) and tests/test_gpu_qa.py."""
import numpy as np
import torch
import torch.nn.functional as F

from ivos_w_amd import metrics

THR = 205


def quantize(p):
    """q = clamp(rint(float32(p * 255)), 0, 255), NaN -> 0: numpy's float32 product, round half to even, the saturating 8-bit cast."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint(p * np.float32(255.0))
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, 0, 255).astype(np.uint8)


def quantize_probs(all_P, n_objects):
    """[n, O+1, H, W] float32 -> uint8 [O, n, H, W], objects 1 .. O (channel 0 is not looked at)."""
    a = all_P.detach().cpu().numpy() if isinstance(all_P, torch.Tensor) else np.asarray(all_P)
    return np.ascontiguousarray(quantize(a[:, 1:n_objects + 1]).transpose(1, 0, 2, 3))


def value_grid():
    """float32 values that decide the quantiser: for every byte k the values just below, at and just above (k + 0.5) / 255 - the ties of
    round half to even and their neighbours - and the specials."""
    vals = []
    for k in range(256):
        c = np.float32((k + 0.5) / 255.0)
        vals += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)), np.float32(k / 255.0)]
    vals += [-0.0, 0.0, -1e-9, -0.3, -5.0, 1.0, 1.0000001, 1.002, 2.0, 300.0, 3e38, np.inf, -np.inf, np.nan, 1e-45, 0.8, 0.80000001,
             204.5 / 255, 205.5 / 255]
    return np.asarray(vals, dtype=np.float32)


def fill(shape, rng=None):
    """A float32 array of `shape` that walks the value grid (cyclically, from a random offset per row when rng is given)."""
    g = value_grid()
    n = int(np.prod(shape))
    start = 0 if rng is None else int(rng.integers(0, g.size))
    return g[(start + np.arange(n) * 7) % g.size].reshape(shape).astype(np.float32)


def unit_targets(counts, metric):
    """counts int64 [N, O, 6] (the count pass's order) -> (target float64 [O * N], valid uint8 [O * N]) in the assessment's unit order
    (object-major), with metrics.py's host expressions."""
    counts = np.asarray(counts)
    j, f = metrics._jaccard_from(counts), metrics._f_from(counts)
    t = j if metric == "J" else f if metric == "F" else .5 * j + .5 * f
    return np.ascontiguousarray(t.T).reshape(-1), np.ascontiguousarray((counts[..., 1] > 0).T).reshape(-1).astype(np.uint8)


def report(scores, target, valid):
    """The reference loop restated in numpy float32: -> (loss, diff, n_valid) as float32, float32, int."""
    s, t = np.asarray(scores, np.float32).reshape(-1), np.asarray(target, np.float64).astype(np.float32).reshape(-1)
    loss, diff, n = np.float32(0), np.float32(0), 0
    for u in range(s.size):
        if valid[u]:
            e = np.float32(s[u] - t[u])
            loss = np.float32(loss + np.float32(e * e))
            diff = np.float32(diff + np.float32(abs(e)))
            n += 1
    if n == 0:
        return np.float32(0), np.float32(0), 0
    return np.float32(loss / np.float32(n)), np.float32(diff / np.float32(n)), n


def reference_loop(scores, target, valid):
    """What quality_assessment.py:249-263 computes, with torch on the CPU and its two expressions per sample: the target as
    torch.from_numpy(metric).float(), F.mse_loss and (pred - gt).abs().mean() on 0-d fp32 tensors, accumulated in sample order over the
    samples whose union is not empty, each total divided by their number (a Python int)."""
    pred = torch.as_tensor(np.asarray(scores, np.float32).reshape(-1))
    gt = torch.from_numpy(np.asarray(target, np.float64).reshape(-1)).float()
    kept = [u for u in range(pred.numel()) if valid[u] > 0]
    if not kept:
        return np.float32(0), np.float32(0), 0
    sq, ab = 0., 0.
    for u in kept:
        sq = sq + F.mse_loss(pred[u], gt[u])
        ab = ab + (pred[u] - gt[u]).abs().mean()
    return np.float32((sq / len(kept)).item()), np.float32((ab / len(kept)).item()), len(kept)
