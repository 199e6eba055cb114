"""Shared by tests/test_jf_videos_option.py (CPU) and tests/test_gpu_jf_videos.py: hand-made J / F count sextets that reach every branch
of the reduce rule, the host path they are held to (metrics._jaccard_from / _f_from + ndarray.mean(axis=1), as sequence_metric combines
them) and a pure-Python restatement of that rule - the definition ivosw_jf_reduce_ragged implements."""
import numpy as np

from ivos_w_amd import metrics

OBJECT_COUNTS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32)
METRICS = ("J", "F", "J_AND_F")

# inter, union, n_fg (pred boundary), n_gt, fg_match, gt_match
SPECIAL = [
    (0, 0, 0, 0, 0, 0),                                       # empty union; no boundary on either side: precision = recall = 1
    (3, 7, 0, 5, 0, 2),                                       # no pred boundary: precision 1, recall 0
    (3, 7, 5, 0, 2, 0),                                       # no gt boundary: precision 0, recall 1
    (5, 9, 11, 13, 7, 3),                                     # the general branch
    (1, 3, 11, 13, 0, 0),                                     # precision + recall == 0
    (2 ** 33 + 1, 2 ** 35 + 7, 3 * 2 ** 31 + 5, 2 ** 32 + 3, 2 ** 31 + 1, 2 ** 32 + 1),       # counts above 2^31
    (2 ** 53 + 1, 2 ** 54 + 3, 2 ** 53 + 3, 2 ** 53 + 5, 2 ** 53 + 1, 2 ** 52 + 1),            # ... and above 2^53: int -> float64 rounds
    (0, 4, 6, 6, 6, 6),                                       # J = 0, F = 1
    (1, 3, 3, 7, 1, 2),                                       # thirds and sevenths: inexact ratios, an inexact product and quotient
]


def make_counts(n_frames, n_obj, seed):
    """int64 [n_frames, n_obj, 6]: random plausible sextets with the SPECIAL ones spread over every object column."""
    rng = np.random.default_rng(seed)
    union = rng.integers(1, 5000, (n_frames, n_obj))
    inter = (union * rng.random((n_frames, n_obj))).astype(np.int64)
    n_fg, n_gt = rng.integers(1, 400, (n_frames, n_obj)), rng.integers(1, 400, (n_frames, n_obj))
    c = np.stack([inter, union, n_fg, n_gt, (n_fg * rng.random((n_frames, n_obj))).astype(np.int64),
                  (n_gt * rng.random((n_frames, n_obj))).astype(np.int64)], -1).astype(np.int64)
    flat = c.reshape(-1, 6)
    for i, s in enumerate(SPECIAL):
        flat[(i * 5 + seed) % len(flat)] = s
    return c


def min_frames(n_obj):
    """Enough frames that every SPECIAL sextet has a slot of its own."""
    return max(2, -(-len(SPECIAL) * 5 // n_obj) + 1)


def host_metric(counts, metric, average=True):
    """What sequence_metric makes of the counts: the host path (utils/misc.py + metrics.py)."""
    if metric == "J":
        j = metrics._jaccard_from(counts)
        return j.mean(axis=1) if average else j
    if metric == "F":
        f = metrics._f_from(counts)
        return f.mean(axis=1) if average else f
    j, f = metrics._jaccard_from(counts), metrics._f_from(counts)
    if average:
        j, f = j.mean(axis=1), f.mean(axis=1)
    return .5 * j + .5 * f


# ------------------------------------------------------------------------------------------------ the restatement
def jaccard_one(c):
    return 1.0 if c[1] == 0 else float(c[0]) / float(c[1])


def f_one(c):
    n_fg, n_gt, m_fg, m_gt = (int(c[k]) for k in (2, 3, 4, 5))
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = float(m_fg) / float(n_fg), float(m_gt) / float(n_gt)
    s = precision + recall
    if s == 0.0:
        return 0.0
    twice = 2.0 * precision
    prod = twice * recall
    return prod / s


def row_mean(v):
    """numpy's add.reduce along a contiguous float64 row of at most 32 elements, then one division."""
    n = len(v)
    if n < 8:
        total = v[0]
        for x in v[1:]:
            total = total + x
    else:
        r = list(v[:8])
        i = 8
        while i + 8 <= n:
            for j in range(8):
                r[j] = r[j] + v[i + j]
            i += 8
        total = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            total = total + v[i]
            i += 1
    return total / float(n)


def restated(counts, metric, average=True):
    n_frames, n_obj = counts.shape[:2]
    out = np.empty((n_frames, n_obj) if not average else (n_frames,), dtype=np.float64)
    for f in range(n_frames):
        rows = [[int(x) for x in counts[f, o]] for o in range(n_obj)]
        j = [jaccard_one(c) for c in rows] if metric != "F" else None
        fm = [f_one(c) for c in rows] if metric != "J" else None
        if not average:
            out[f] = j if metric == "J" else fm if metric == "F" else [.5 * a + .5 * b for a, b in zip(j, fm)]
        elif metric == "J":
            out[f] = row_mean(j)
        elif metric == "F":
            out[f] = row_mean(fm)
        else:
            out[f] = .5 * row_mean(j) + .5 * row_mean(fm)
    return out
