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


# ------------------------------------------------------------------------------------------------ assessment samples: 8-bit planes, per-unit targets
QA_THRESHOLD = 205                       # byte / 255 > 0.8 (quality_assessment.py:235) first holds at 205, in float64 and in float32


def _quantize_launch(p, n_objects, out):
    """One ivosw_qa_quantize launch: ``p`` a float32 device tensor indexed [n, O+1, H, W] whose planes are contiguous (any frame / channel
    strides), ``out`` uint8 [O, n, H, W]."""
    n, C, H, W = (int(d) for d in p.shape)
    stride_n = int(p.stride(0)) if n > 1 else H * W            # (the stride of an extent-1 dimension is arbitrary in torch)
    L.check(L.lib().ivosw_qa_quantize(L.C.c_void_p(p.data_ptr()), n, n_objects, H, W, stride_n, int(p.stride(1)),
                                      L.dptr(out, torch.uint8), L.stream_ptr(p.device)), "qa_quantize")
    return out


def quantize_probs(all_P, n_objects):
    """``all_P`` -> device uint8 [O, n, H, W], object-major, objects 1 .. O (channel 0 is never read): the bytes the reference's
    ``save_seg_preds`` writes, q = clamp(rint(float32(p * 255)), 0, 255), formed where all_P lives (``ivosw_qa_quantize``, one launch, no
    synchronisation).  ``all_P``: a float32 device tensor indexed [n, O+1, H, W] - the reference's layout or the permuted view of an
    object-major store, both without a copy - or a ProbStore / AtnetStore / IpnStore (its ``all_P``); a host numpy array is uploaded first."""
    p = all_P.all_P if hasattr(all_P, "all_P") else all_P
    if isinstance(p, np.ndarray):
        p = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(_device())
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise RuntimeError("quantize_probs: all_P must live on the GPU (a device tensor, a store, or a numpy array to upload): no CPU fallback")
    if p.ndim != 4 or p.dtype != torch.float32:
        raise ValueError(f"quantize_probs: all_P must be float32 [n, O+1, H, W], got {p.dtype} {tuple(p.shape)}")
    n, C, H, W = (int(d) for d in p.shape)
    n_objects = int(n_objects)
    if n_objects < 1 or n_objects + 1 > C:
        raise ValueError(f"quantize_probs: {n_objects} objects do not fit all_P's {C} channels (channel 0 is the background)")
    if n == 0 or H * W == 0:
        raise ValueError("quantize_probs: empty all_P")
    if (W > 1 and p.stride(3) != 1) or (H > 1 and p.stride(2) != W) or (n > 1 and p.stride(0) < H * W) or p.stride(1) < H * W:
        p = p.contiguous()                                  # planes that are not contiguous: one copy, then the reference layout
    return _quantize_launch(p, n_objects, torch.empty((n_objects, n, H, W), dtype=torch.uint8, device=p.device))


class QaTargets:
    """What ``qa_targets`` leaves on the device, flat over the videos in the assessment's unit order (video-major, inside a video
    object-major: unit = first_unit[v] + obj * N_v + frame).  ``target`` float64 [units], ``valid`` uint8 [units] (union > 0), ``counts``
    int64 [units * 6] in the count pass's order (frame-major inside a video); with scores ``report`` float32 [V, 3] = (loss, diff,
    n_valid) per video - ``loss`` / ``diff`` / ``n_valid`` are its sources - else None.  ``views``: one [O_v, N_v] view of target per video."""

    def __init__(self, target, valid, counts, loss, diff, n_valid, lengths, n_obj):
        self.target, self.valid, self.counts, self.loss, self.diff, self.n_valid = target, valid, counts, loss, diff, n_valid
        self.lengths, self.n_obj = lengths, n_obj
        offs = np.concatenate([[0], np.cumsum([n * o for n, o in zip(lengths, n_obj)])]).astype(np.int64)
        self.unit_off = offs
        self.views = [target[int(offs[i]):int(offs[i + 1])].view(n_obj[i], lengths[i]) for i in range(len(lengths))]
        self.valid_views = [valid[int(offs[i]):int(offs[i + 1])].view(n_obj[i], lengths[i]) for i in range(len(lengths))]

    @property
    def report(self):
        if self.loss is None:
            return None
        return torch.stack([self.loss, self.diff, self.n_valid.to(torch.float32)], 1)


def qa_counts(videos, thr=QA_THRESHOLD, bound_th=0.008):
    """The six integer counts per (frame, object) with the prediction taken from byte planes (``ivosw_qa_counts_videos``): ``videos`` =
    [(gt_labels [N,H,W], planes_u8 [O,N,H,W], n_objects[, obj_ids]), ...].  Returns (counts int64 device [pairs * 6], lengths, n_obj); one
    memset + two launches per group of videos, split as ``jf_videos`` splits them; no synchronisation."""
    videos = list(videos)
    if not videos:
        raise ValueError("qa_counts needs at least one video")
    thr = int(thr)
    if not 0 <= thr <= 255:
        raise ValueError(f"thr must be a byte, got {thr}")
    dev = next((t.device for v in videos for t in v[:2] if isinstance(t, torch.Tensor) and t.is_cuda), None) or _device()
    lib, st = L.lib(), L.stream_ptr(dev)
    keep, descs = [], []
    for i, video in enumerate(videos):
        y_true, planes, nb_objects = video[:3]
        ids = video[3] if len(video) > 3 and video[3] is not None else None
        gt = _as_labels(y_true, dev)
        if isinstance(planes, np.ndarray):
            planes = torch.from_numpy(np.ascontiguousarray(planes))
        pl = (planes if planes.is_cuda else planes.to(dev)).contiguous()
        if gt.ndim != 3:
            raise ValueError(f"video {i}: the label map must have 3 dimensions, found {gt.ndim}")
        if pl.dtype != torch.uint8 or pl.ndim != 4:
            raise ValueError(f"video {i}: planes must be uint8 [O, N, H, W], got {pl.dtype} {tuple(pl.shape)}")
        ids = np.asarray([k + 1 for k in range(int(nb_objects))] if ids is None else list(ids), dtype=np.int64)
        if len(ids) == 0 or len(ids) > 32 or ids.min() < 0 or ids.max() > 255:
            raise ValueError(f"video {i}: 1..32 object ids in 0..255")
        if tuple(pl.shape) != (len(ids),) + tuple(gt.shape):
            raise ValueError(f"video {i}: planes {tuple(pl.shape)} do not match {len(ids)} objects x label map {tuple(gt.shape)}")
        N, H, W = (int(d) for d in gt.shape)
        bp = bound_pixels((H, W), bound_th)
        if bp != int(bp) or bp > 32:
            raise ValueError(f"boundary tolerance {bp} px: the kernel supports integer radii up to 32")
        keep.append((gt, pl))                                             # (alive until the launches are enqueued)
        d = L.QaVideo(gt=gt.data_ptr(), planes=pl.data_ptr(), n_frames=N, H=H, W=W, n_obj=len(ids), bound_pix=int(bp), thr=thr)
        for k, v in enumerate(ids):
            d.obj_ids[k] = int(v)
        descs.append(d)
    lengths, n_obj = [d.n_frames for d in descs], [d.n_obj for d in descs]
    pair_off = np.concatenate([[0], np.cumsum([n * o for n, o in zip(lengths, n_obj)])]).astype(np.int64)
    counts = torch.empty(int(pair_off[-1]) * 6, dtype=torch.int64, device=dev)
    for a, b in _jf_groups(list(zip(lengths, n_obj))):
        table = (L.QaVideo * (b - a))(*descs[a:b])
        nbytes = lib.ivosw_qa_counts_ws_bytes(table, b - a)
        key = (dev.index, "jf")
        ws = _ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _ws[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        L.check(lib.ivosw_qa_counts_videos(table, b - a, L.dptr(counts[int(pair_off[a]) * 6:int(pair_off[b]) * 6], torch.int64),
                                           L.dptr(ws, torch.uint8), ws.numel(), st), "qa_counts_videos")
    return counts, lengths, n_obj


def qa_targets_from_counts(counts, lengths, n_obj, metric, scores=None):
    """``ivosw_qa_targets`` over flat counts: one launch per L.MAX_SEQS videos.  ``scores``: None, a flat float32 device tensor in unit
    order, or one [O_v, N_v] tensor per video (concatenated).  Returns a ``QaTargets``; no synchronisation."""
    if metric not in METRIC_CODES:
        raise ValueError(f"metric must be one of {sorted(METRIC_CODES)}, got {metric!r}")
    dev = counts.device
    lib, st = L.lib(), L.stream_ptr(dev)
    unit_off = np.concatenate([[0], np.cumsum([n * o for n, o in zip(lengths, n_obj)])]).astype(np.int64)
    units, V = int(unit_off[-1]), len(lengths)
    if counts.numel() != units * 6:
        raise ValueError(f"counts has {counts.numel()} entries for {units} units")
    if scores is not None:
        if not isinstance(scores, torch.Tensor):
            scores = torch.cat([s.reshape(-1) for s in scores])
        scores = scores.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        if scores.numel() != units:
            raise ValueError(f"scores has {scores.numel()} entries for {units} units")
    target = torch.empty(units, dtype=torch.float64, device=dev)
    valid = torch.empty(units, dtype=torch.uint8, device=dev)
    loss = diff = n_valid = None
    if scores is not None:
        loss, diff = torch.empty(V, dtype=torch.float32, device=dev), torch.empty(V, dtype=torch.float32, device=dev)
        n_valid = torch.empty(V, dtype=torch.int32, device=dev)
    for a in range(0, V, L.MAX_SEQS):
        b = min(a + L.MAX_SEQS, V)
        u0, u1 = int(unit_off[a]), int(unit_off[b])
        L.check(lib.ivosw_qa_targets(
            L.dptr(counts[u0 * 6:u1 * 6], torch.int64), L.int_array(n_obj[a:b]), L.int_array(lengths[a:b]), b - a, METRIC_CODES[metric],
            L.dptr(scores[u0:u1]) if scores is not None else None, L.dptr(target[u0:u1], torch.float64), L.dptr(valid[u0:u1], torch.uint8),
            L.dptr(loss[a:b]) if loss is not None else None, L.dptr(diff[a:b]) if diff is not None else None,
            L.dptr(n_valid[a:b], torch.int32) if n_valid is not None else None, st), "qa_targets")
    return QaTargets(target, valid, counts, loss, diff, n_valid, list(lengths), list(n_obj))


def qa_targets(videos, metric, scores=None, thr=QA_THRESHOLD, bound_th=0.008):
    """AssessNet's per-sample targets on the device (quality_assessment.py:235-263): ``videos`` = [(gt_labels, planes_u8, n_objects[,
    obj_ids]), ...] with planes_u8 the [O,N,H,W] bytes of ``quantize_probs``; per unit (object, frame) the mask is ``plane >= thr``
    (205 = the reference's ``byte / 255 > 0.8``), the ground truth ``label == obj_id``, the target J, F or .5 J + .5 F of that unit alone
    and ``valid`` = the union is not empty.  With ``scores`` (the session's per-unit AssessNet scores) also the reference loop's ``loss``
    (mean squared error) and ``diff`` (mean absolute error) over each video's valid units, in its fp32 summation order.  Returns a
    ``QaTargets`` of device tensors and does not synchronise."""
    if metric not in METRIC_CODES:
        raise ValueError(f"metric must be one of {sorted(METRIC_CODES)}, got {metric!r}")
    counts, lengths, n_obj = qa_counts(videos, thr, bound_th)
    return qa_targets_from_counts(counts, lengths, n_obj, metric, scores)
