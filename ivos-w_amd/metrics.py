"""DAVIS J / F metrics on the device — drop-in for ``davisinteractive.metrics.batched_jaccard`` /
``batched_f_measure`` as the reference's ``sequence_metric`` uses them (utils/misc.py:118-162).

The label maps go to the GPU once (or already live there as the VOS model's argmax output); two kernels
(``csrc/metrics.hip``) return six integer counts per (frame, object), and the float64 ratios are formed here with the
package's own expressions — so J and F equal the CPU implementation bit for bit whenever the counts do.
There is no CPU fallback: without the HIP library or a GPU the call raises.

``jf_videos`` scores several videos in one pass and forms the ratios and the per-frame means on the device as well
(``ivosw_jf_counts_videos``, ``ivosw_jf_reduce_ragged``): nothing comes back to the host, so the oracle setting's chain
(``utils_agent.oracle_recommend``) runs from the label maps to the recommended frames with one copy.
"""
import numpy as np
import torch

from . import _lib as L

_ws = {}


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("ivos_w_amd.metrics: no GPU — the J/F kernels have no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _as_labels(a, dev):
    """[N,H,W] integer labels (numpy or tensor, any integer dtype) -> contiguous uint8 device tensor."""
    if isinstance(a, torch.Tensor):
        t = a if a.is_cuda else a.to(dev, non_blocking=True)
        if t.dtype != torch.uint8:
            t = t.to(torch.uint8)
        return t.contiguous()
    a = np.asarray(a)
    if a.dtype != np.uint8:
        if a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("label maps must hold values in 0..255")
        a = a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(y_true, y_pred):
    if y_true.ndim != 3:
        raise ValueError(f"y_true array must have 3 dimensions. Found {y_true.ndim} dimensions")
    if y_pred.ndim != 3:
        raise ValueError(f"y_pred array must have 3 dimensions. Found {y_pred.ndim} dimensions")
    if tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError(f"y_true and y_pred must have the same shape. {tuple(y_true.shape)} != {tuple(y_pred.shape)}")


def _object_ids(gt, nb_objects):
    if nb_objects is None:
        ids = torch.unique(gt)
        ids = ids[(ids < 255) & (ids > 0)].cpu().numpy().astype(np.int64)
    else:
        ids = np.asarray([i + 1 for i in range(nb_objects)], dtype=np.int64)
    if len(ids) == 0:
        raise ValueError("Number of objects in y_true should be higher than 0.")
    return ids


def bound_pixels(shape, bound_th=0.008):
    return bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape))


def jf_counts(y_true, y_pred, nb_objects=None, bound_th=0.008):
    """-> (ids [O], counts int64 [N,O,6]): |gt&pred|, |gt|pred|, #pred-boundary, #gt-boundary, matched pred, matched gt."""
    _check(y_true, y_pred)
    dev = y_true.device if isinstance(y_true, torch.Tensor) and y_true.is_cuda else _device()
    gt, pr = _as_labels(y_true, dev), _as_labels(y_pred, dev)
    ids = _object_ids(gt, nb_objects)
    if ids.max() > 255:
        raise ValueError("object ids above 255 cannot occur in uint8 label maps")
    N, H, W = gt.shape
    bp = bound_pixels((H, W), bound_th)
    if bp != int(bp) or bp > 32:
        raise ValueError(f"boundary tolerance {bp} px: the kernel supports integer radii up to 32")
    lib = L.lib()
    counts = torch.empty((N, len(ids), 6), dtype=torch.int64, device=dev)
    nbytes = lib.ivosw_jf_ws_bytes(N, H, W, len(ids))
    key = (dev.index, "jf")
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idb = bytes(ids.astype(np.uint8).tolist())
    L.check(lib.ivosw_jf_counts(L.dptr(gt, torch.uint8), L.dptr(pr, torch.uint8), N, H, W, idb, len(ids), int(bp),
                                L.dptr(counts, torch.int64), L.dptr(ws, torch.uint8), nbytes, L.stream_ptr(dev)), "jf_counts")
    return ids, counts.cpu().numpy()


def _jaccard_from(counts):
    inter, union = counts[..., 0], counts[..., 1]
    out = np.empty(inter.shape, dtype=np.float64)
    for idx in np.ndindex(inter.shape):
        out[idx] = 1.0 if np.isclose(union[idx], 0) else inter[idx] / union[idx]
    return out


def _f_from(counts):
    out = np.empty(counts.shape[:-1], dtype=np.float64)
    for idx in np.ndindex(out.shape):
        n_fg, n_gt, m_fg, m_gt = (counts[idx][k] for k in (2, 3, 4, 5))
        if n_fg == 0 and n_gt > 0:
            precision, recall = 1, 0
        elif n_fg > 0 and n_gt == 0:
            precision, recall = 0, 1
        elif n_fg == 0 and n_gt == 0:
            precision, recall = 1, 1
        else:
            precision = m_fg / float(n_fg)
            recall = m_gt / float(n_gt)
        out[idx] = 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return out


def batched_jaccard(y_true, y_pred, average_over_objects=True, nb_objects=None):
    _, counts = jf_counts(y_true, y_pred, nb_objects)
    j = _jaccard_from(counts)
    return j.mean(axis=1) if average_over_objects else j


def batched_f_measure(y_true, y_pred, average_over_objects=True, nb_objects=None, bound_th=0.008):
    _, counts = jf_counts(y_true, y_pred, nb_objects, bound_th)
    f = _f_from(counts)
    return f.mean(axis=1) if average_over_objects else f


def batched_j_and_f(y_true, y_pred, average_over_objects=True, nb_objects=None, bound_th=0.008):
    """Both metrics from ONE pass over the label maps (the reference runs the two functions back to back)."""
    _, counts = jf_counts(y_true, y_pred, nb_objects, bound_th)
    j, f = _jaccard_from(counts), _f_from(counts)
    if average_over_objects:
        j, f = j.mean(axis=1), f.mean(axis=1)
    return j, f


# ------------------------------------------------------------------------------------------------ several videos, ratios on the device
METRIC_CODES = {"J": L.METRIC_J, "F": L.METRIC_F, "J_AND_F": L.METRIC_J_AND_F}
GRID_LIMIT = 65535                       # a flat grid dimension of ivosw_jf_counts_videos: frames, and (frame, object) pairs, per group


class JfVideos:
    """What ``jf_videos`` leaves on the device.  ``quality``: float64 [R], flat over the videos (R = all frames); ``views``: one [N_v]
    view of it per video; ``state``: float32 [R,2] = (float32(quality), annot_counts) or None; ``per_object``: one float64 [N_v,O_v] view
    per video of the un-averaged values, or None; ``lengths`` / ``n_obj``: N_v and O_v."""

    def __init__(self, quality, views, state, per_object, lengths, n_obj, per_object_flat=None):
        self.quality, self.views, self.state, self.per_object, self.lengths, self.n_obj = quality, views, state, per_object, lengths, n_obj
        self.per_object_flat = per_object_flat                # the tensor the per_object views slice (one copy fetches them all)


def _jf_groups(shapes):
    """[(start, stop)] over videos of (N, O): at most L.MAX_JF_VIDEOS videos, GRID_LIMIT frames and GRID_LIMIT (frame, object) pairs each."""
    groups, start, frames, pairs = [], 0, 0, 0
    for i, (n, o) in enumerate(shapes):
        if n > GRID_LIMIT or n * o > GRID_LIMIT:
            raise ValueError(f"video {i}: {n} frames x {o} objects do not fit one grid dimension ({GRID_LIMIT}): split the sequence")
        if i - start == L.MAX_JF_VIDEOS or frames + n > GRID_LIMIT or pairs + n * o > GRID_LIMIT:
            groups.append((start, i))
            start, frames, pairs = i, 0, 0
        frames += n
        pairs += n * o
    if len(shapes) > start:
        groups.append((start, len(shapes)))
    return groups


def jf_videos(videos, metric, annot_counts=None, per_object=False, bound_th=0.008, out=None):
    """J / F / J&F of SEVERAL videos in one device pass, the ratios and the mean over the objects included: ``videos`` is a sequence of
    (y_true, y_pred, nb_objects) - [N,H,W] label maps, numpy or device tensors under ``jf_counts``'s rules, each video its own size;
    ``metric`` one of "J", "F", "J_AND_F".  Returns a ``JfVideos`` of DEVICE tensors and does not synchronise (with nb_objects given: None
    looks the ids up in y_true, which reads them back): one memset + two launches per group of videos (ivosw_jf_counts_videos: up to
    L.MAX_JF_VIDEOS videos and GRID_LIMIT frames / (frame, object) pairs a group) and one ivosw_jf_reduce_ragged launch per L.MAX_SEQS
    videos.  ``annot_counts`` ([R] annotation counts, numpy or tensor): also fill the Brain's state.  ``per_object``: also keep the
    un-averaged values.  ``out`` (float64 device tensor, >= R elements): the quality is written to its head.  Per video the values equal
    ``utils.misc.sequence_metric`` on that video, bit for bit."""
    if metric not in METRIC_CODES:
        raise ValueError(f"metric must be one of {sorted(METRIC_CODES)}, got {metric!r}")
    videos = list(videos)
    if not videos:
        raise ValueError("jf_videos needs at least one video")
    dev = next((t.device for v in videos for t in v[:2] if isinstance(t, torch.Tensor) and t.is_cuda), None) or _device()
    lib, st = L.lib(), L.stream_ptr(dev)
    maps, descs = [], []
    for y_true, y_pred, nb_objects in videos:
        _check(y_true, y_pred)
        gt, pr = _as_labels(y_true, dev), _as_labels(y_pred, dev)
        ids = _object_ids(gt, nb_objects)
        if ids.max() > 255:
            raise ValueError("object ids above 255 cannot occur in uint8 label maps")
        N, H, W = (int(d) for d in gt.shape)
        bp = bound_pixels((H, W), bound_th)
        if bp != int(bp) or bp > 32:
            raise ValueError(f"boundary tolerance {bp} px: the kernel supports integer radii up to 32")
        maps.append((gt, pr))                                             # (alive until the launches are enqueued)
        d = L.JfVideo(gt=gt.data_ptr(), pred=pr.data_ptr(), n_frames=N, H=H, W=W, n_obj=len(ids), bound_pix=int(bp))
        for i, v in enumerate(ids):
            d.obj_ids[i] = int(v)
        descs.append(d)
    lengths, n_obj = [d.n_frames for d in descs], [d.n_obj for d in descs]
    pair_off = np.concatenate([[0], np.cumsum([n * o for n, o in zip(lengths, n_obj)])]).astype(np.int64)
    row_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    R, pairs = int(row_off[-1]), int(pair_off[-1])
    counts = torch.empty(pairs * 6, dtype=torch.int64, device=dev)
    for a, b in _jf_groups(list(zip(lengths, n_obj))):
        table = (L.JfVideo * (b - a))(*descs[a:b])
        nbytes = lib.ivosw_jf_videos_ws_bytes(table, b - a)
        key = (dev.index, "jf")
        ws = _ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _ws[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        L.check(lib.ivosw_jf_counts_videos(table, b - a, L.dptr(counts[int(pair_off[a]) * 6:int(pair_off[b]) * 6], torch.int64),
                                           L.dptr(ws, torch.uint8), ws.numel(), st), "jf_counts_videos")
    if out is not None:
        if out.dtype != torch.float64 or not out.is_cuda or out.numel() < R or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float64 device tensor of at least {R} elements")
        quality = out.view(-1)[:R]
    else:
        quality = torch.empty(R, dtype=torch.float64, device=dev)
    state = cnt = None
    if annot_counts is not None:
        cnt = annot_counts if isinstance(annot_counts, torch.Tensor) else torch.as_tensor(np.asarray(annot_counts, dtype=np.float32))
        cnt = cnt.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        if cnt.numel() != R:
            raise ValueError(f"annot_counts has {cnt.numel()} entries for {R} frames")
        state = torch.empty(R, 2, dtype=torch.float32, device=dev)
    per = torch.empty(pairs, dtype=torch.float64, device=dev) if per_object else None
    for a in range(0, len(descs), L.MAX_SEQS):
        b = min(a + L.MAX_SEQS, len(descs))
        r0, r1, p0, p1 = int(row_off[a]), int(row_off[b]), int(pair_off[a]), int(pair_off[b])
        L.check(lib.ivosw_jf_reduce_ragged(
            L.dptr(counts[p0 * 6:p1 * 6], torch.int64), L.int_array(n_obj[a:b]), L.int_array(lengths[a:b]), b - a, METRIC_CODES[metric],
            L.dptr(cnt[r0:r1]) if cnt is not None else None, L.dptr(per[p0:p1]) if per is not None else None,
            L.dptr(quality[r0:r1], torch.float64), L.dptr(state[r0:r1]) if state is not None else None, st), "jf_reduce_ragged")
    views = [quality[int(row_off[i]):int(row_off[i + 1])] for i in range(len(descs))]
    per_views = None
    if per is not None:
        per_views = [per[int(pair_off[i]):int(pair_off[i + 1])].view(lengths[i], n_obj[i]) for i in range(len(descs))]
    return JfVideos(quality, views, state, per_views, lengths, n_obj, per)
