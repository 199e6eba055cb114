"""Recommendation glue around the hot path — drop-in for the reference's ``utils.utils_agent``.

Function names, argument meaning and return values follow /root/reference/utils/utils_agent.py
(``goal_only_reward`` :7-35, ``select_next_frame`` :38-74, ``recommend_frame`` :77-128, ``gen_subseq`` :131-157,
``agent_train_data_collection`` :160-204, ``agent_business`` :207-256).  What changed is where the data lives:
in the wild/ours and wild/worst branches the video is uploaded ONCE per sequence and cached on the GPU, all objects of a
sequence are scored by one batched AssessNet pass that reads every object's mask in place and shares one copy of the frames
(the reference runs one forward per object and copies the video H2D every interaction, :114-119), and mask quality ->
state -> Brain -> argmax runs on the device; one small D2H copy returns the quality vector and the recommended index.
"""
import copy

import numpy as np
import torch


def goal_only_reward(sequence, n_interaction, scribble_iter, repeat_selection, iou_new, df=None):
    """reward_step = +1 / -1 (repeat selection); reward_done = (mean(J&F) - mu - sigma) / sigma against the 30
    random-policy baselines stored in reward.csv (ddof=1)."""
    reward_step = np.array(-1) if repeat_selection else np.array(1)
    if df is None:
        return reward_step, np.array(0)
    rows = df[(df.sequence == sequence) & (df.n_interaction_next == n_interaction)]
    rows = rows[((rows.scribble_iter - 1) % 3) == ((scribble_iter - 1) % 3)]
    baseline = np.array([np.mean([float(tok) for tok in s.split("/")]) for s in rows.next_state_iou])
    assert len(baseline) == 30
    mu, sigma = baseline.mean(), baseline.std(ddof=1)
    return reward_step, (iou_new.mean() - mu - sigma) / sigma


def select_next_frame(frame_value, metric="min", prev_frames=None):
    """'random' | 'worst'/'min' (lowest value not yet annotated) | 'max' (negates, like the reference) | 'prob'."""
    n = len(frame_value)
    if metric == "random":
        return int(np.random.randint(n, size=1)[0])
    if metric == "uniform":
        assert prev_frames is not None
    if metric == "prob":
        draw = np.random.rand()
        prob = torch.softmax(torch.Tensor(frame_value), 0)
        k = 0
        while draw > 0:
            draw = draw - prob[k]
            k += 1
        return k - 1
    if metric == "max":
        frame_value = -frame_value
    if prev_frames is None:
        return frame_value.argmin()
    for idx in frame_value.argsort():
        if idx not in prev_frames:
            return idx
    return frame_value.argmin()          # every frame already annotated


def gen_subseq(first_frame, n_frame, len_subseq, subseq_style="consecutive"):
    if subseq_style == "consecutive":
        assert n_frame >= len_subseq
        lo = max(0, first_frame - len_subseq + 1)
        hi = first_frame - max(first_frame + len_subseq - n_frame, 0)
        start = int((lo + hi) / 2)
        return list(range(start, start + len_subseq))
    if subseq_style == "equal":
        if n_frame < len_subseq + 1:
            return list(np.array(range(len_subseq)))
        grid = np.linspace(0, n_frame - 1, num=len_subseq + 1).astype(int)
        while first_frame not in list(grid):
            grid += 1
        return list(grid[:-1]) if first_frame != grid[-1] else list(grid[1:])
    raise NotImplementedError


def _annotation_counts(n, annotated_frames_list):
    counts = np.zeros(n)
    for i in annotated_frames_list:
        counts[i] += 1
    return counts


def _topk_options(cfg_yl, agent):
    """(k, skip_annotated, gap): the agent's checked options; without an agent (method "worst" needs none) cfg.agent's keys, defaults
    1 / False / 1.  The gap (agent.candidate_gap) is the one the k candidates are spread by: 1 with one candidate, where it has no effect."""
    from ..models.agent import candidate_gap_option, candidates_option
    if agent is not None and hasattr(agent, "candidates"):
        k, skip = candidates_option(agent.candidates, agent.skip_annotated)
        gap = candidate_gap_option(getattr(agent, "candidate_gap", 1))
    else:
        a = cfg_yl.get("agent") if hasattr(cfg_yl, "get") else None
        if a is None:
            return 1, False, 1
        k, skip = candidates_option(a.get("candidates", 1), a.get("skip_annotated", False))
        gap = candidate_gap_option(a.get("candidate_gap", 1))
    return k, skip, gap if k > 1 else 1


def worst_candidates(frame_value, k, prev_frames=None, gap=1):
    """The first k frames of the order select_next_frame(frame_value, "worst", prev_frames) walks: its pick, then the other frames that are
    not in prev_frames by rising value, then (when those run out) the frames of prev_frames by rising value.  np.int64 [min(k, n)].
    With `gap` > 1 the order is walked greedily (agent.candidate_gap, the rule of ivosw_brain_topk_spread_ragged): a frame is accepted only
    `gap` or more frames from every accepted one, and the list is shorter than k when no more can be."""
    first = int(select_next_frame(frame_value, metric="worst", prev_frames=prev_frames))
    order = [int(i) for i in np.asarray(frame_value).argsort() if int(i) != first]
    if prev_frames is not None:
        order = [i for i in order if i not in prev_frames] + [i for i in order if i in prev_frames]
    if gap > 1:
        taken = []
        for t in [first] + order:
            if len(taken) < k and all(abs(t - w) >= gap for w in taken):
                taken.append(t)
        return np.array(taken, dtype=np.int64)
    return np.array([first] + order, dtype=np.int64)[:k]


def _candidate_list(pick, k):
    """What a k = 1 recommendation returns (one index) or a k > 1 one (an array), as the np.int64 array recommend_candidates returns."""
    return np.atleast_1d(np.asarray(pick, dtype=np.int64))[:k]


def _first(pick):
    """Candidate 0 of what Agent.action returns: the index itself with agent.candidates = 1, else the first entry of its array."""
    return pick[0] if np.ndim(pick) else pick


class _FrameCache:
    """The video of the current sequence, resident on the GPU across interactions.  The reference uploads all_F (and all_P)
    on EVERY interaction (utils/utils_agent.py:114-115: 100 frames x 480p fp32 = 0.5 GB, ~10 ms of PCIe per call); the entry
    scripts build all_F once per sequence (eval_agent_manet.py:297-300), so its identity is a sound cache key.  One entry: the
    previous sequence's host frames (~0.5 GB) stay alive until the next sequence replaces them, or ``clear_frame_cache()``."""

    def __init__(self):
        self.key, self.src, self.frames, self.uploads, self.hits = None, None, None, 0, 0

    def get(self, all_F, device):
        device = torch.device(device)
        if _is_packed(all_F):                    # 8-bit frames already packed on the device (pack_video): handed on unchanged
            return all_F
        if all_F.is_cuda:
            return all_F if all_F.device == device else all_F.to(device)
        # The cache holds a STRONG reference to the host tensor and compares identity: while the entry is alive the tensor cannot be
        # freed, so the allocator cannot hand its address to the next sequence's frames (same shape, same version counter) and make
        # a stale entry look current.  (data_ptr stays in the key for a tensor object whose storage was swapped with .set_() / .data.)
        key = (all_F.data_ptr(), tuple(all_F.shape), all_F.dtype, all_F._version, str(device))
        if self.src is not all_F or key != self.key:
            self.frames = all_F.to(device=device, dtype=torch.float32).contiguous()
            self.key, self.src = key, all_F
            self.uploads += 1
        else:
            self.hits += 1
        return self.frames

    def clear(self):
        self.key, self.src, self.frames = None, None, None


def _is_packed(all_F):
    from ..models.assessment import PackedFrames
    return isinstance(all_F, PackedFrames)


def _is_labels(all_P):
    from ..models.assessment import LabelMasks
    return isinstance(all_P, LabelMasks)


def _masks_on(all_P, device):
    """all_P - a float tensor or a LabelMasks (masks=labels) - on ``device``: handed on when it is there, uploaded when it is not."""
    device = torch.device(device)
    if _is_labels(all_P):
        return all_P.to(device)
    return all_P if (all_P.is_cuda and all_P.device == device) else all_P.to(device)


def pack_video(u8, device, layout="hwc"):
    """The decoded 8-bit frames of a video ([n,H,W,3], or [n,3,H,W] with layout="chw"; torch or numpy uint8, host or device) ->
    ``models.assessment.PackedFrames`` on ``device``: a quarter of the fp32 video's bytes over PCIe and in HBM.  Hand the result to
    ``recommend_frame`` / ``assess_all_objects`` / ``AssessNet`` in place of the float all_F; the scores equal those of u8 / 255."""
    from ..models.assessment import pack_frames
    return pack_frames(u8, device, layout)


frame_cache = _FrameCache()


def clear_frame_cache():
    """Drop the cached video (call when a host all_F buffer is rewritten in place through numpy, which does not bump the
    tensor version the cache key watches)."""
    frame_cache.clear()


RESCORE_MODES = ("all", "changed")
# score_cache keeps the sessions' plane copies and score tables up to this many bytes (least recently used first out).  One 100-frame,
# 3-object 480p session costs 0.49 GB (300 planes of 480 x 854 fp32), or 41 MB with label-map masks (100 uint8 maps).
SCORE_CACHE_BYTES = 8 << 30


def rescore_option(cfg):
    """cfg.rescore (absent: "all"), refused unless it is one of RESCORE_MODES.  "changed": the assessment pass scores only the (frame,
    object) units whose masks changed since the session was last scored (AssessNet.forward_videos_incremental); same results."""
    mode = (cfg.get("rescore", "all") if hasattr(cfg, "get") else getattr(cfg, "rescore", "all")) if cfg is not None else "all"
    if not isinstance(mode, str) or mode not in RESCORE_MODES:
        raise ValueError(f"rescore must be 'all' or 'changed', got {mode!r}")
    return mode


def _video_dims(all_F):
    """(n_frames, H, W) of a float all_F or a PackedFrames."""
    if _is_packed(all_F):
        return all_F.n, all_F.H, all_F.W
    return int(all_F.shape[0]), int(all_F.shape[2]), int(all_F.shape[3])


class _ScoreCacheLRU:
    """The sessions' ScoreCaches under rescore=changed, least recently used first out, bounded by SCORE_CACHE_BYTES.  Keyed like a
    ScoreCache - the frames object's identity (the entry's ScoreCache holds the strong reference once it was used), n_frames, n_obj, H,
    W, the net's precision and weights key - plus the video's rank among the videos of one call that share that key (two requests on one
    frames object get a cache each; which one a request meets decides how much is scored again, never what comes out).
    ``units`` / ``rescored``: totals over all calls (``stats()`` brings them up to date)."""

    def __init__(self):
        from collections import OrderedDict
        self.entries = OrderedDict()
        self.units, self._rescored, self._pending = 0, 0, []

    def get_many(self, assess_net, videos):
        """One ScoreCache per (all_F, all_P, n_objects) of a call, made on first sight; the ones handed out become the most recent."""
        from ..models.assessment import ScoreCache
        out, seen = [], {}
        for all_F, all_P, n_objects in videos:             # (all_P is looked at for its kind only: a LabelMasks or not)
            n, H, W = _video_dims(all_F)
            kind = "labels" if _is_labels(all_P) else "float32"
            key, _ = ScoreCache.make_key(assess_net, all_F, n, int(n_objects), H, W, kind)
            rank = seen[key] = seen.get(key, -1) + 1
            entry = self.entries.get((key, rank))
            if entry is None or (entry[0].src is not None and entry[0].src is not all_F):
                entry = (ScoreCache(), ScoreCache.nbytes_for(n, int(n_objects), H, W, kind))
            self.entries[(key, rank)] = entry
            self.entries.move_to_end((key, rank))
            out.append(entry[0])
        return out

    def nbytes(self):
        return sum(b for _, b in self.entries.values())

    def trim(self, limit=None):
        """Evict least recently used entries until the rest fits `limit` bytes (default SCORE_CACHE_BYTES)."""
        limit = SCORE_CACHE_BYTES if limit is None else limit
        while self.entries and self.nbytes() > limit:
            _, (cache, _) = self.entries.popitem(last=False)
            cache.clear()

    def account(self, caches):
        for c in caches:
            self.units += c.units
            if isinstance(c._rescored, torch.Tensor):
                self._pending.append(c._rescored)            # counted on the device: fetched by stats(), not here (no extra sync)
            else:
                self._rescored += c._rescored
        if len(self._pending) > 256:
            self._pending = [torch.stack(self._pending).sum()]
        self.trim()

    def stats(self):
        """(units seen, units scored again) over all calls so far."""
        for t in self._pending:
            self._rescored += int(t.item())
        self._pending = []
        return self.units, self._rescored

    @property
    def rescored(self):
        return self.stats()[1]

    def clear(self):
        for cache, _ in self.entries.values():
            cache.clear()
        self.entries.clear()
        self.units, self._rescored, self._pending = 0, 0, []


score_cache = _ScoreCacheLRU()


def clear_score_cache():
    """Drop every cached score table and plane copy (rescore=changed).  Call when a video's frames are rewritten IN PLACE behind an
    unchanged tensor object - through numpy or .data, which do not bump the tensor version the key watches: the masks are compared on the
    device on every call, the frames are not.  (The same caveat as clear_frame_cache.)"""
    score_cache.clear()


def _forward_changed(assess_net, on_dev, sources):
    """forward_videos through the score caches: on_dev = the device-resident (frames, probs, n_objects), sources = the callers' all_F."""
    caches = score_cache.get_many(assess_net, [(src, v[1] if _is_labels(v[1]) else None, v[2]) for src, v in zip(sources, on_dev)])
    out = assess_net.forward_videos_incremental(on_dev, caches, sources=sources)
    score_cache.account(caches)
    return out


def assess_all_objects_device(assess_net, all_F, all_P, n_objects, device, rescore="all"):
    """[n_objects, n_frame] quality predictions ON the device from one launch sequence: every object's masks are read in
    place from all_P (channel i+1 = object i) and all objects share one device copy of the frames (frame-index
    indirection inside ivosw_assess_forward_objects) - nothing is repeated, transposed or copied.
    rescore="changed": only the units whose masks changed since this video was last scored are scored again (score_cache); same values."""
    frames = frame_cache.get(all_F, device)
    probs = _masks_on(all_P, device)                     # (a LabelMasks - masks=labels - travels in all_P's place)
    if rescore == "changed":
        return _forward_changed(assess_net, [(frames, probs, n_objects)], [all_F])[0]
    return assess_net.forward_objects(frames, probs, n_objects)


def assess_all_objects(assess_net, all_F, all_P, n_objects, device, rescore="all"):
    """[n_frame, n_objects] quality predictions as a host array (one small D2H copy)."""
    return assess_all_objects_device(assess_net, all_F, all_P, n_objects, device, rescore).transpose(0, 1).cpu().numpy()


# The per-unit scores of the assessment passes, for a caller that reports on them (entry's qa_report): None (the default: nothing is
# kept, nothing is launched), or a list that _wild_assess / _recommend_many append one [n_objects, n_frame] device copy per video to.
score_tap = None


def _tap(scores):
    if score_tap is not None:
        score_tap.append(scores.detach().clone())


def assess_report(videos, scores, metric, thr=None, bound_th=0.008):
    """How far AssessNet's scores are from the truth, as the reference's training loop measures it (quality_assessment.py:235-263), in one
    device chain: ``videos`` = [(gt_labels [N,H,W], all_P | store | quantised uint8 planes [O,N,H,W], n_objects), ...], ``scores`` the
    session's per-unit scores (one [O, N] device tensor per video, as ``assess_videos_device`` returns them, or one flat tensor).
    metrics.quantize_probs (one launch per float video) -> the count pass from the byte planes (one memset, two launches) ->
    ivosw_qa_targets (one launch) -> ONE copy of [loss, diff, n_valid] per video.  Returns (report float32 numpy [V, 3], QaTargets)."""
    from .. import metrics
    thr = metrics.QA_THRESHOLD if thr is None else thr
    table = []
    for gt, probs, n_objects in videos:
        planes = probs if (isinstance(probs, torch.Tensor) and probs.dtype == torch.uint8) else metrics.quantize_probs(probs, n_objects)
        table.append((gt, planes, n_objects))
    res = metrics.qa_targets(table, metric, scores=scores, thr=thr, bound_th=bound_th)
    return res.report.cpu().numpy(), res                                  # the one D2H copy of the call


def assess_report_augmented(videos, assess_net, metric, transform=None, seed=None, batch=32, thr=None, bound_th=0.008):
    """``assess_report`` on ONE augmented copy of every unit, as an AssessNet training step would see it, without leaving the device:
    datasets.transforms_assess (one fused warp per batch of ``batch`` samples) -> ``assess_net.forward(img, prob)`` -> the count pass on
    (label, mask) as a 1-object video of N frames -> ivosw_qa_targets -> ONE copy of [loss, diff, n_valid].
    ``videos`` = [(frames (float32 device tensor | PackedFrames | host tensor), gt_labels [N,H,W], all_P | store | uint8 planes [O,N,H,W],
    n_objects), ...], all of one frame size unless ``transform`` resizes; the units run video-major, object-major, frame-minor.
    ``transform``: a transforms_assess.Compose (default: the reference's train pipeline at the first video's size).  ``seed``: the host
    streams (``random``, ``np.random``) are seeded with it for the draws and put back afterwards; None draws from them as they are.
    Returns (report float32 numpy [1, 3] = loss, diff, n_valid over all units, QaTargets)."""
    import random as _random
    from .. import metrics
    from ..datasets import transforms_assess as T
    thr = metrics.QA_THRESHOLD if thr is None else thr
    device = next(assess_net.parameters()).device
    table, samples = [], []
    for v, (frames, gt, probs, n_objects) in enumerate(videos):
        if not _is_packed(frames) and not frames.is_cuda:
            frames = frame_cache.get(frames, device)
        planes = probs if (isinstance(probs, torch.Tensor) and probs.dtype == torch.uint8) else metrics.quantize_probs(probs, n_objects)
        gt = metrics._as_labels(gt, device)
        table.append((frames, gt, planes.to(device).contiguous()))
        samples += [(v, f, o) for o in range(int(n_objects)) for f in range(int(gt.shape[0]))]
    if transform is None:
        transform = T.train_transform(size=(int(table[0][1].shape[2]), int(table[0][1].shape[1])))
    state = None
    if seed is not None:
        state = (_random.getstate(), np.random.get_state())
        _random.seed(int(seed))
        np.random.seed(int(seed) % (1 << 32))
    try:
        scores, labels, masks = [], [], []
        for a in range(0, len(samples), batch):
            out = transform(T.DeviceSamples(table, samples[a:a + batch]))
            scores.append(assess_net.forward(out["img"], out["prob"]).reshape(-1))
            labels.append(out["label"])
            masks.append(out["mask"])
    finally:
        if state is not None:
            _random.setstate(state[0])
            np.random.set_state(state[1])
    label, mask = torch.cat(labels), torch.cat(masks)
    res = metrics.qa_targets([(label, mask[None], 1)], metric, scores=torch.cat(scores), thr=thr, bound_th=bound_th)
    return res.report.cpu().numpy(), res                                  # the one D2H copy of the call


def _assess_bank(videos, assess_net, metric, transform, copies, batch, thr, bound_th):
    """``copies`` passes of ``transform`` over every unit of ``videos`` (the tuples of ``assess_report_augmented``) through
    ``assess_net.forward_features`` and the count pass: (scores [copies * U], features [copies * U, 2048], QaTargets, U), row = copy * U +
    unit, all on the device, no synchronisation.  The caller seeds the host streams."""
    from .. import metrics
    from ..datasets import transforms_assess as T
    device = next(assess_net.parameters()).device
    table, samples = [], []
    for v, (frames, gt, probs, n_objects) in enumerate(videos):
        if not _is_packed(frames) and not frames.is_cuda:
            frames = frame_cache.get(frames, device)
        planes = probs if (isinstance(probs, torch.Tensor) and probs.dtype == torch.uint8) else metrics.quantize_probs(probs, n_objects)
        gt = metrics._as_labels(gt, device)
        table.append((frames, gt, planes.to(device).contiguous()))
        samples += [(v, f, o) for o in range(int(n_objects)) for f in range(int(gt.shape[0]))]
    size = (int(table[0][1].shape[2]), int(table[0][1].shape[1]))
    if transform is None:
        transform = T.train_transform(size=size)
    elif transform == "plain":
        transform = T.Compose([T.Resize(size=size), T.ToTensor()])
    scores, feats, labels, masks = [], [], [], []
    for _ in range(copies):
        for a in range(0, len(samples), batch):
            out = transform(T.DeviceSamples(table, samples[a:a + batch]))
            sc, ft = assess_net.forward_features(out["img"], out["prob"])
            scores.append(sc)
            feats.append(ft)
            labels.append(out["label"])
            masks.append(out["mask"])
    scores = torch.cat(scores)
    res = metrics.qa_targets([(torch.cat(labels), torch.cat(masks)[None], 1)], metric, scores=scores, thr=thr, bound_th=bound_th)
    return scores, torch.cat(feats), res, len(samples)


def head_fit_options(cfg):
    """The ``assess_net`` keys of a head fit, checked: -> dict(lrs, momentum, weight_decay, gamma, num_epochs, train_batch_size, zero_grad,
    augment_copies, val_fraction).  ``cfg`` is the whole config or its ``assess_net`` block.  ``fit`` must be ``head``: training the trunk
    is outside this path (it runs with folded BatchNorm, which cannot represent it)."""
    from .. import _lib as L
    a = cfg["assess_net"] if "assess_net" in cfg else cfg
    fit = a.get("fit", "head")
    if fit != "head":
        raise ValueError(f"assess_net.fit={fit!r}: only 'head' is accepted - trunk training is outside this path (the tower runs with "
                         "folded BatchNorm; fc1 is fitted on the pooled features of the frozen trunk)")
    lr = a.get("lr", 5e-6)
    lrs = [float(v) for v in lr] if isinstance(lr, (list, tuple)) else [float(lr)]
    if not lrs or any(not (v > 0 and np.isfinite(v)) for v in lrs):
        raise ValueError(f"assess_net.lr must be a positive number or a non-empty list of them, got {lr!r}")
    o = dict(lrs=lrs, momentum=float(a.get("momentum", 0.9)), weight_decay=float(a.get("weight_decay", 5e-4)), gamma=float(a.get("gamma", 0.95)),
             num_epochs=int(a.get("num_epochs", 50)), train_batch_size=int(a.get("train_batch_size", 32)), zero_grad=a.get("zero_grad", True),
             augment_copies=int(a.get("augment_copies", 1)), val_fraction=float(a.get("val_fraction", 0.1)))
    if isinstance(o["zero_grad"], str):
        if o["zero_grad"].lower() not in ("true", "false"):
            raise ValueError(f"assess_net.zero_grad must be true or false, got {o['zero_grad']!r}")
        o["zero_grad"] = o["zero_grad"].lower() == "true"
    o["zero_grad"] = bool(o["zero_grad"])
    if not 0 <= o["momentum"] < 1 or o["weight_decay"] < 0 or not 0 < o["gamma"] <= 1:
        raise ValueError("assess_net: momentum in [0, 1), weight_decay >= 0 and gamma in (0, 1] are required")
    if o["num_epochs"] < 1 or o["augment_copies"] < 1:
        raise ValueError("assess_net.num_epochs and assess_net.augment_copies must be at least 1")
    if not 1 <= o["train_batch_size"] <= L.HEAD_FIT_MAX_BATCH:
        raise ValueError(f"assess_net.train_batch_size must be 1 .. {L.HEAD_FIT_MAX_BATCH}, got {o['train_batch_size']}")
    if not 0 <= o["val_fraction"] < 1:
        raise ValueError(f"assess_net.val_fraction must be in [0, 1), got {o['val_fraction']}")
    return o


def fit_assess_head(videos, assess_net, metric, cfg, transform=None, seed=None, thr=None, bound_th=0.008, log=print, bank_out=None):
    """Calibrate AssessNet's score head to a VOS back end: ``videos`` as ``assess_report_augmented`` takes them.  Draws
    ``assess_net.augment_copies`` augmented copies of every unit in batches of ``train_batch_size`` -> ``forward_features`` ->
    ``metrics.qa_targets`` into one feature bank on the device; holds out ``val_fraction`` of the UNITS (all copies of a held-out unit);
    ``AssessNet.fit_head`` (ivosw_head_fit: every epoch of every config in one launch) with the reference's hyper-parameters - a list in
    ``assess_net.lr`` is a sweep, the config with the lowest held-out loss wins; ``set_head``.  Returns dict(before, after: loss, diff, n
    on the un-augmented units; chosen: the config; result: the HeadFitResult; holdout: the chosen config's held-out loss, diff, n).
    ``bank_out``: a dict that receives the bank (features, target, valid, holdout rows as host numpy) - for tests and post-mortems."""
    import random as _random
    from .. import metrics
    o = head_fit_options(cfg)
    thr = metrics.QA_THRESHOLD if thr is None else thr
    seed = 2019 if seed is None else int(seed)            # the reference's set_random_seed(2019)
    state = (_random.getstate(), np.random.get_state())
    _random.seed(seed)
    np.random.seed(seed % (1 << 32))
    try:
        plain = lambda: _assess_bank(videos, assess_net, metric, "plain", 1, o["train_batch_size"], thr, bound_th)[2].report
        before = plain()
        _, feats, res, U = _assess_bank(videos, assess_net, metric, transform, o["augment_copies"], o["train_batch_size"], thr, bound_th)
    finally:
        _random.setstate(state[0])
        np.random.set_state(state[1])
    n_hold = int(round(o["val_fraction"] * U))
    if o["val_fraction"] > 0 and U >= 2:
        n_hold = min(max(n_hold, 1), U - 1)
    held_units = np.sort(np.random.RandomState(seed).permutation(U)[:n_hold])
    holdout = (np.arange(o["augment_copies"])[:, None] * U + held_units[None]).reshape(-1) if n_hold else None
    rows = o["augment_copies"] * (U - n_hold)
    batch = min(o["train_batch_size"], rows)
    if batch != o["train_batch_size"]:
        log(f"fit_assess_head: {rows} training rows: the batch is {batch}, not train_batch_size={o['train_batch_size']}")
    log(f"fit_assess_head: fit=head, {o['augment_copies']} x {U} units ({n_hold} held out), {len(o['lrs'])} config(s), "
        + ("zero_grad=true (plain SGD)" if o["zero_grad"] else "zero_grad=false (the reference's accumulating clamped gradients)"))
    target32 = res.target.to(torch.float32)
    if bank_out is not None:
        bank_out.update(features=feats.cpu().numpy(), target=target32.cpu().numpy(), valid=res.valid.cpu().numpy(),
                        holdout=None if holdout is None else holdout.copy(), batch_size=batch, seed=seed,
                        w0=assess_net.fc1.weight.detach().cpu().numpy().reshape(-1).copy(), b0=float(assess_net.fc1.bias.detach().cpu()))
    fit = assess_net.fit_head(feats, target32, res.valid, lr=o["lrs"][0], momentum=o["momentum"], weight_decay=o["weight_decay"],
                              gamma=o["gamma"], num_epochs=o["num_epochs"], batch_size=batch, seed=seed, zero_grad=o["zero_grad"],
                              configs=[dict(lr=v) for v in o["lrs"]], holdout=holdout)
    assess_net.set_head(*fit.chosen())
    after = plain()
    rep = torch.cat([before, after]).cpu().numpy()                      # [loss, diff, n] before | after
    as_dict = lambda r: dict(loss=float(r[0]), diff=float(r[1]), n=int(r[2]))
    out = dict(before=as_dict(rep[0]), after=as_dict(rep[1]), chosen=dict(fit.configs[fit.best], index=fit.best), result=fit, holdout=None)
    if fit.holdout_n is not None:
        out["holdout"] = dict(loss=float(fit.holdout_loss[fit.best]), diff=float(fit.holdout_diff[fit.best]), n=int(fit.holdout_n[fit.best]))
    return out


def _wild_assess(method, assess_net, agent, device, n_objects, all_F, all_P, counts, mask_quality, prev_frames, k=1, as_list=False,
                 rescore="all", gap=1):
    """wild/worst and wild/ours (utils/utils_agent.py:111-122) with the chain quality -> state -> Brain -> argmax on the
    device: per-object scores are averaged into mask_quality (float64, numpy's summation order) and stacked with the
    annotation counts by ivosw_quality_state, the Brain and its first-max argmax read that state in place, and ONE D2H copy
    brings back the n quality values the caller's array wants plus the recommended index.  With agent.candidates = k /
    agent.skip_annotated the argmax is the masked top-k and the buffer holds k indices; `as_list`: return all candidates (an array).
    With `gap` > 1 (agent.candidate_gap) the device ranking is the spread one and final: it is not merged with the random pick again."""
    from .. import _lib as L
    from ..models.agent import merge_candidates, spread_candidates
    scores = assess_all_objects_device(assess_net, all_F, all_P, n_objects, device, rescore)
    _tap(scores)
    n = scores.shape[1]
    dev = scores.device
    out = torch.empty(n + k, dtype=torch.float64, device=dev)          # [quality (n) | k recommended indices (int64 bits)]
    state = torch.empty(n, 2, dtype=torch.float32, device=dev)
    cnt = torch.as_tensor(np.asarray(counts, dtype=np.float32)).to(dev, non_blocking=True)
    L.check(L.lib().ivosw_quality_state(L.dptr(scores), n_objects, n, L.dptr(cnt), L.dptr(out), L.dptr(state),
                                        L.stream_ptr(dev)), "quality_state")
    idx_dev = out[n:].view(torch.int64)
    idx_dev.zero_()
    picked = agent.action(state, device_out=idx_dev) if method == "ours" else None
    host = out.cpu()                                                    # the one D2H copy of the interaction
    mask_quality[:] = host[:n].numpy()          # in place: the caller logs corr/diff from this array
    if method == "worst":
        if as_list:
            return worst_candidates(mask_quality, k, prev_frames, gap)
        return select_next_frame(mask_quality, metric="worst", prev_frames=prev_frames)
    if k > 1:
        ranking = host[n:].view(torch.int64).numpy()
        cand = spread_candidates(ranking) if gap > 1 else merge_candidates(picked, ranking, k)
        return cand if as_list else cand[0]
    pick = picked if picked is not None else np.int64(host[n:].view(torch.int64)[0].item())
    return _candidate_list(pick, 1) if as_list else pick


def assess_videos_device(assess_net, videos, device, rescore="all"):
    """Quality predictions of SEVERAL videos from one assessment pass (AssessNet.forward_videos): ``videos`` is a sequence of
    (all_F | PackedFrames, all_P | LabelMasks, n_objects); returns one [n_objects, n_frame] device tensor per video, each bit for bit what
    ``assess_all_objects_device`` gives for that video alone.  Host-resident tensors are uploaded for this call only: the single-entry
    ``frame_cache`` is neither read nor written (several videos would evict each other on every call) - multi-session callers keep
    their videos on the device (``pack_video``, or ``all_F.to(device)`` once per sequence).
    rescore="changed": only the units whose masks changed since each video was last scored are scored again (score_cache, keyed by the
    all_F object the caller hands in); same values."""
    device = torch.device(device)
    on_dev, sources = [], []
    for all_F, all_P, n_objects in videos:
        sources.append(all_F)
        if not _is_packed(all_F) and not (all_F.is_cuda and all_F.device == device):
            all_F = all_F.to(device=device, dtype=torch.float32)
        on_dev.append((all_F, _masks_on(all_P, device), n_objects))
    if rescore == "changed":
        return _forward_changed(assess_net, on_dev, sources)
    return assess_net.forward_videos(on_dev)


# recommend_frames runs quality -> state -> Brain -> argmax as ONE ragged chain from this many requests on, and per request below it.
# tools/ragged_brain_probe.py times both chains (profiles/ragged_brain_probe.txt): at 2 requests of 30 frames 170 us per request against
# 117 us ragged with a run-to-run spread of 3 us (100 frames: 261 against 159, spread 23), and the gap grows with every request.
RAGGED_MIN_REQUESTS = 2


def recommend_frames(cfg_yl, assess_net, agent, device, requests):
    """``recommend_frame`` for several sessions at once: ``requests`` is a sequence of dicts, each the keyword arguments of
    ``recommend_frame`` behind ``device`` (n_frame, n_objects, all_F, all_P, new_masks_quality, prev_frames, annotated_frames_list,
    mask_quality, first_frame, max_nb_interactions).  Returns the recommended indices in request order.

    Under wild/ours and wild/worst all requests share ONE assessment pass (assess_videos_device: K short videos fill one full-size pass
    instead of K small ones) and, from RAGGED_MIN_REQUESTS requests on, ONE chain behind it whatever K is: one upload of the concatenated
    counts, ivosw_quality_state_ragged over the flat scores of that pass (every request's float64 quality and fp32 state in one launch),
    ``agent.actions`` (the host work of ``agent.action`` per request in request order - ``steps_done`` and the host RNG move exactly as
    under sequential ``recommend_frame`` calls - then ONE ragged Brain forward over all sessions, each of its own length, and ONE ragged
    first-max argmax: five launches where the per-request loop needed 5 K, and the K recurrences run side by side instead of one behind
    the other), and ONE device-to-host copy of [quality (R) float64 | index (K) int64] that fills each request's ``mask_quality`` in
    place.  A single request keeps the per-request chain.  Indices and quality vectors equal those of ``recommend_frame`` per request,
    bit for bit.  Every other setting / method is ``recommend_frame`` per request.

    With agent.candidates = k / agent.skip_annotated the chain ends in the ragged masked top-k instead of the argmax (still five launches
    and one copy, of [quality (R) | K k indices]); the index returned per request is candidate 0 (``recommend_candidates`` returns all).

    Keep the videos on the device (``pack_video`` or ``all_F.to(device)`` once per sequence): host-resident frames are uploaded on
    every call here, and the single-entry ``frame_cache`` of ``recommend_frame`` is left alone."""
    return _recommend_many(cfg_yl, assess_net, agent, device, requests, as_list=False)


def recommend_candidates(cfg_yl, assess_net, agent, device, requests):
    """``recommend_frames`` with every candidate returned: one np.int64 array of min(agent.candidates, n_frame) frame indices per request,
    the strongest first (entry 0 is what ``recommend_frames`` returns), and the same in-place ``mask_quality`` side effect.  One request
    or many: the same chains as ``recommend_frames`` (a single request takes the per-request chain with a one-sequence top-k).  wild/ours
    and oracle/ours: Agent.action's candidates (the ranking by Q, annotated frames last under agent.skip_annotated; on the epsilon branch
    the random pick first); oracle/ours runs on the host state.  "worst": the first k frames of the order select_next_frame walks
    (``worst_candidates``).  "random" / "linspace": their single pick.

    With agent.candidate_gap = g > 1 the candidates of a request lie g or more frames apart (the order above walked greedily; on the device
    ivosw_brain_topk_spread_ragged in the top-k's place, the random pick of the epsilon branch its forced first candidate): the list may
    be shorter than k, entry 0 is what it is without a gap, and the chains keep their launches and their one copy."""
    return _recommend_many(cfg_yl, assess_net, agent, device, requests, as_list=True)


def _recommend_many(cfg_yl, assess_net, agent, device, requests, as_list):
    requests = list(requests)
    k, _, gap = _topk_options(cfg_yl, agent)
    if not (cfg_yl.setting == "wild" and cfg_yl.method in ("worst", "ours")):
        if as_list:
            return [_recommend_one(cfg_yl, assess_net, agent, device, k=k, as_list=True, gap=gap, **r) for r in requests]
        return [recommend_frame(cfg_yl, assess_net, agent, device, **r) for r in requests]
    if as_list and len(requests) == 1:           # one session: recommend_frame's chain (its frame cache, a one-sequence top-k)
        return [_recommend_one(cfg_yl, assess_net, agent, device, k=k, as_list=True, gap=gap, **requests[0])]
    if not requests:
        return []
    from .. import _lib as L
    from ..models.agent import merge_candidates, spread_candidates
    method = cfg_yl.method
    K = len(requests)
    with torch.no_grad():
        scores = assess_videos_device(assess_net, [(r["all_F"], r["all_P"], r["n_objects"]) for r in requests], device, rescore_option(cfg_yl))
        for s in scores:
            _tap(s)
        dev = scores[0].device
        ns = [int(s.shape[1]) for s in scores]
        counts = [_annotation_counts(len(r["new_masks_quality"]), r["annotated_frames_list"]) for r in requests]
        cnt = torch.as_tensor(np.concatenate(counts).astype(np.float32)).to(dev, non_blocking=True)      # one upload for all requests
        if K < RAGGED_MIN_REQUESTS:
            qoffs = np.concatenate([[0], np.cumsum([n + k for n in ns])])[:-1]   # per request [quality (n) | k recommended indices (int64 bits)]
            ioffs = [int(o) + n for o, n in zip(qoffs, ns)]
            out = torch.zeros(sum(ns) + K * k, dtype=torch.float64, device=dev)
            picked, c0 = [], 0
            for r, s, n, o in zip(requests, scores, ns, qoffs):
                o = int(o)
                state = torch.empty(n, 2, dtype=torch.float32, device=dev)
                L.check(L.lib().ivosw_quality_state(L.dptr(s), int(r["n_objects"]), n, L.dptr(cnt[c0:c0 + n]), L.dptr(out[o:o + n]),
                                                    L.dptr(state), L.stream_ptr(dev)), "quality_state")
                c0 += n
                picked.append(agent.action(state, device_out=out[o + n:o + n + k].view(torch.int64)) if method == "ours" else None)
        else:
            R = sum(ns)
            qoffs = np.concatenate([[0], np.cumsum(ns)])[:-1]                    # [quality of every request (R) | the K k indices (int64 bits)]
            ioffs = [R + j * k for j in range(K)]
            out = torch.zeros(R + K * k, dtype=torch.float64, device=dev)
            state = torch.empty(R, 2, dtype=torch.float32, device=dev)
            for g in range(0, K, L.MAX_SEQS):                                    # (one launch per 128 requests)
                o, n_g = int(qoffs[g]), sum(ns[g:g + L.MAX_SEQS])
                L.check(L.lib().ivosw_quality_state_ragged(
                    L.dptr(scores[g]), L.int_array(int(s.shape[0]) for s in scores[g:g + L.MAX_SEQS]), L.int_array(ns[g:g + L.MAX_SEQS]),
                    len(ns[g:g + L.MAX_SEQS]), L.dptr(cnt[o:o + n_g]), L.dptr(out[o:o + n_g]), L.dptr(state[o:o + n_g]), L.stream_ptr(dev)),
                    "quality_state_ragged")
            picked = [None] * K
            if method == "ours":
                picked = agent.actions([state[int(o):int(o) + n] for o, n in zip(qoffs, ns)], device_out=out[R:].view(torch.int64))
        host = out.cpu()                                                    # the one D2H copy of the call
    quality, index = host.numpy(), host.view(torch.int64).numpy()
    result = []
    for r, n, o, i, pk in zip(requests, ns, qoffs, ioffs, picked):
        o = int(o)
        r["mask_quality"][:] = quality[o:o + n]                             # in place: the caller logs corr/diff from this array
        if method == "worst":
            result.append(worst_candidates(r["mask_quality"], k, r["prev_frames"], gap) if as_list else
                          select_next_frame(r["mask_quality"], metric="worst", prev_frames=r["prev_frames"]))
        elif k > 1:                                                         # (a spread ranking is final: the pick is its slot 0 already)
            cand = spread_candidates(index[i:i + k]) if gap > 1 else merge_candidates(pk, index[i:i + k], k)
            result.append(cand if as_list else cand[0])
        else:
            pick = pk if pk is not None else np.int64(index[i])
            result.append(_candidate_list(pick, 1) if as_list else pick)
    return result


def recommend_frame(cfg_yl, assess_net, agent, device, n_frame, n_objects, all_F, all_P, new_masks_quality, prev_frames,
                    annotated_frames_list, mask_quality, first_frame, max_nb_interactions):
    k, _, gap = _topk_options(cfg_yl, agent)
    return _recommend_one(cfg_yl, assess_net, agent, device, n_frame, n_objects, all_F, all_P, new_masks_quality, prev_frames,
                          annotated_frames_list, mask_quality, first_frame, max_nb_interactions, k=k, as_list=False, gap=gap)


def _recommend_one(cfg_yl, assess_net, agent, device, n_frame, n_objects, all_F, all_P, new_masks_quality, prev_frames,
                   annotated_frames_list, mask_quality, first_frame, max_nb_interactions, k=1, as_list=False, gap=1):
    """recommend_frame (the reference's index: candidate 0), or with `as_list` the candidates of recommend_candidates (`gap` apart)."""
    setting, method = cfg_yl.setting, cfg_yl.method
    one = (lambda pick: _candidate_list(pick, k)) if as_list else _first
    if setting == "oracle":
        if method == "worst":
            if as_list:
                return worst_candidates(new_masks_quality, k, prev_frames, gap)
            return select_next_frame(new_masks_quality, metric="worst", prev_frames=prev_frames)
        if method == "ours":
            state = np.stack([new_masks_quality, _annotation_counts(len(new_masks_quality), annotated_frames_list)], 1)
            with torch.no_grad():
                return one(agent.action(state))
        raise NotImplementedError
    if setting == "wild":
        if method == "random":
            return one(select_next_frame(new_masks_quality, metric="random"))
        if method == "linspace":
            subseq = gen_subseq(first_frame, n_frame, min(max_nb_interactions, n_frame), "equal")
            return one(next((i for i in subseq if i not in prev_frames), prev_frames[0]))
        if method in ("worst", "ours"):
            counts = _annotation_counts(len(new_masks_quality), annotated_frames_list)
            with torch.no_grad():
                return _wild_assess(method, assess_net, agent, device, n_objects, all_F, all_P, counts, mask_quality,
                                    prev_frames, k=k, as_list=as_list, rescore=rescore_option(cfg_yl), gap=gap)
        raise NotImplementedError
    raise NotImplementedError


def agent_train_data_collection(agent, reward_step, reward_done, annotated_frames_list_np, next_annotated_frames_list_np,
                                old_masks_IoU, new_masks_IoU, old_masks_meta, new_masks_meta, done, old_frame,
                                report_save_dir):
    """Serialise the per-frame vectors as '/'-joined str(float) lists (the memory_pool.csv cell format) and push."""
    join = lambda seq: "/".join(str(v) for v in seq)
    n = len(old_masks_IoU)
    agent.memory(old_masks_meta, old_frame, new_masks_meta, reward_step, reward_done, done,
                 join(old_masks_IoU[i] for i in range(n)), join(new_masks_IoU[i] for i in range(n)),
                 join(annotated_frames_list_np[i] for i in range(n)),
                 join(next_annotated_frames_list_np[i] for i in range(n)), report_save_dir)


def agent_business(cfg_yl, agent, max_nb_interactions, n_interaction, first_scribble, old_masks_metric, new_masks_metric,
                   old_frame, sequence, seen_seq, repeat_selection, df, annotated_frames_list, next_frame, old_masks_meta,
                   new_masks_meta, report_save_dir, agent_train_loader):
    agent_loss_iter, reward_step, reward_done = np.array(0), np.array(0), np.array(0)
    if first_scribble or cfg_yl.phase == "eval":
        return agent_loss_iter, reward_step, reward_done
    reward_step, reward_done = goal_only_reward(sequence, n_interaction, seen_seq[sequence], repeat_selection,
                                                new_masks_metric, df=df)
    n = len(new_masks_metric)
    nxt = copy.deepcopy(annotated_frames_list)
    nxt.append(next_frame)
    done = n_interaction >= max_nb_interactions
    agent_train_data_collection(agent, reward_step, reward_done, _annotation_counts(n, annotated_frames_list),
                                _annotation_counts(n, nxt), old_masks_metric, new_masks_metric, old_masks_meta,
                                new_masks_meta, done, old_frame, report_save_dir)
    if n_interaction == max_nb_interactions and cfg_yl.phase == "train":
        max_steps = max_nb_interactions * 3 - 1           # at most 3*max_nb_interactions - 1 DQN steps per episode
        losses = _device_update_loop(agent, agent_train_loader, max_steps)
        if losses is None:                                # a foreign loader: the reference's loop, one update_agent per collated batch
            losses = []
            for i, sample in enumerate(agent_train_loader):
                if i == max_steps:
                    break
                losses.append(agent.update_agent(sample))
        agent_loss_iter = np.array(losses).mean()
    return agent_loss_iter, reward_step, reward_done


def _device_update_loop(agent, loader, max_steps):
    """The episode's DQN updates (reference utils/utils_agent.py:244-252) without the per-step host traffic, when the loader is a
    plain DataLoader over this build's own replay dataset (datasets/agent_dataset.py): the dataset's SoA is uploaded once
    (DeviceReplay), the loader's OWN batch sampler supplies the minibatch indices — the same indices, drawn from torch's global
    generator in the same order as iterating the loader would (its base seed first, then the sampler's) — each step gathers its
    minibatch on the device and runs loss + gradients + [all-reduce] + clamp + Adam + the target rule (Agent.target_step: the host coin), and the losses come back in ONE
    device-to-host copy at the end.  Same minibatches, same arithmetic, same coin and RNG streams as ``agent.update_agent(sample)``
    per collated batch: losses, parameters and the agent's loss ring are bit-identical (tests/test_gpu_agent.py).
    Returns the list of losses, or None when the loader is not of that kind (``IVOSW_UPDATE_PATH=host`` forces None).
    Under agent.replay = "prioritized" the minibatches come from the prioritized draw instead (_prioritized_update_loop)."""
    import os
    if getattr(agent, "replay_kind", "uniform") == "prioritized":
        return _prioritized_update_loop(agent, loader, max_steps)
    ds = getattr(loader, "dataset", None)
    bs = getattr(loader, "batch_sampler", None)
    if os.environ.get("IVOSW_UPDATE_PATH", "") == "host" or ds is None or bs is None or not hasattr(ds, "to_device_replay"):
        return None
    if getattr(loader, "num_workers", 0) != 0 or getattr(loader, "collate_fn", None) is not torch.utils.data.default_collate \
            or getattr(ds, "transform", None) is not None or len(ds) == 0:
        return None
    dev = torch.device(agent.device)
    if dev.type != "cuda":
        return None
    replay = getattr(ds, "_device_replay", None)
    if replay is None or replay.device != dev:
        replay = ds._device_replay = ds.to_device_replay(dev)
    # what DataLoader.__iter__ draws from the global generator before the sampler's own seed (torch/utils/data/dataloader.py,
    # _BaseDataLoaderIter.__init__: the base seed), so that the global RNG stream stays the one of the per-batch loop
    torch.empty((), dtype=torch.int64).random_(generator=getattr(loader, "generator", None))
    steps = []
    for i, idx in enumerate(bs):
        if i == max_steps:
            break
        steps.append(list(idx))
    if not steps:
        return []
    flat = torch.as_tensor([j for st in steps for j in st], dtype=torch.int64).to(dev)       # one upload for the whole episode
    loss_dev = torch.empty(len(steps), dtype=torch.float32, device=dev)
    off = 0
    for k, st in enumerate(steps):
        batch = replay.sample(flat[off:off + len(st)])
        off += len(st)
        loss_dev[k:k + 1].copy_(agent.loss_and_grads(batch))
        agent.apply_gradients(check_every=len(steps))
        if agent.target_step():                  # the coin of np.random, or the device rule (agent.target_update)
            print("target_net updated!")
    losses = [float(v) for v in loss_dev.cpu().numpy()]
    for v in losses:
        agent.note_loss(v)
    return losses


def _prioritized_update_loop(agent, loader, max_steps):
    """The episode's DQN updates under agent.replay = "prioritized": one step per batch the loader would have yielded (at most
    max_steps), each = prioritized draw + gather of loader.batch_size rows (PrioritizedReplay.sample_prioritized) -> importance-weighted
    loss and gradients -> clamp + Adam / SGD (apply_gradients) -> priority update from the rows' TD errors -> the target rule
    (Agent.target_step), as in the uniform loop.  The replay is the dataset's own, uploaded once; the first one is seeded from torch's global
    generator, and a reloaded dataset gets the previous tree rebuilt over its rows (PrioritizedReplay.rebuilt: the leaves carry over when
    the old rows are a prefix of the new ones).  Losses come back in one device-to-host copy at the end.
    Refused (ValueError): a loader that is not a plain DataLoader over this build's replay dataset, IVOSW_UPDATE_PATH=host, an initialised
    process group (rank-local TD errors would make the replicas' trees diverge)."""
    import os
    why = None
    ds = getattr(loader, "dataset", None)
    if os.environ.get("IVOSW_UPDATE_PATH", "") == "host":
        why = "IVOSW_UPDATE_PATH=host selects the per-batch host update, which has no prioritized draw"
    elif agent._world()[0] is not None:
        why = "torch.distributed is initialised: data-parallel prioritized replay is not supported (the ranks' trees would diverge)"
    elif ds is None or not hasattr(ds, "to_device_replay") or getattr(loader, "batch_size", None) is None \
            or getattr(loader, "num_workers", 0) != 0 or getattr(loader, "collate_fn", None) is not torch.utils.data.default_collate \
            or getattr(ds, "transform", None) is not None:
        why = "the loader is not a plain DataLoader (batch_size, no workers, no transform) over the agent replay dataset"
    elif torch.device(agent.device).type != "cuda":
        why = "the prioritized replay lives on the GPU"
    if why is not None:
        raise ValueError(f"agent.replay = 'prioritized': {why}")
    if len(ds) == 0:
        return []
    dev = torch.device(agent.device)
    per = getattr(ds, "_per_replay", None)
    if per is None or per.device != dev:
        prev = agent.per_replay
        if prev is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            per = agent.prioritized_replay(ds.soa, dev, seed)
        else:
            per = prev.rebuilt(ds.soa)
        ds._per_replay = agent.per_replay = per
    B = int(loader.batch_size)
    n_steps = min(len(loader), max_steps)
    if n_steps <= 0:
        return []
    batch = per.new_batch(B)
    loss_dev = torch.empty(n_steps, dtype=torch.float32, device=dev)
    for k in range(n_steps):
        per.sample_prioritized(B, out=batch)
        loss_dev[k:k + 1].copy_(agent.loss_and_grads(batch))
        agent.apply_gradients(check_every=n_steps)
        per.update_priorities(batch["idx"], batch["td"])
        if agent.target_step():                  # the coin of np.random, or the device rule (agent.target_update)
            print("target_net updated!")
    losses = [float(v) for v in loss_dev.cpu().numpy()]
    for v in losses:
        agent.note_loss(v)
    return losses


METRIC_MODES = ("host", "device")


def metric_option(cfg):
    """cfg.metric (absent: "host"), refused unless it is one of METRIC_MODES.  "device": the oracle setting scores J / F and recommends in
    one device chain (``oracle_recommend``, ``misc.sequence_metric_videos``) instead of ``sequence_metric`` + ``recommend_frame``; same
    results."""
    mode = (cfg.get("metric", "host") if hasattr(cfg, "get") else getattr(cfg, "metric", "host")) if cfg is not None else "host"
    if not isinstance(mode, str) or mode not in METRIC_MODES:
        raise ValueError(f"metric must be 'host' or 'device', got {mode!r}")
    return mode


# oracle_recommend runs J / F -> state -> Brain -> ranking as ONE device chain from this many sessions on, and sequence_metric +
# recommend_frame per session below it.  tools/jf_videos_probe.py times both (profiles/jf_videos_probe.txt): the one-pass chain is the
# faster one from a single session on, at every condition measured, by more than the run's spread.
ORACLE_MIN_SESSIONS = 1


def _oracle_metric_name(cfg_yl):
    di = cfg_yl.get("davis_interactive") if hasattr(cfg_yl, "get") else getattr(cfg_yl, "davis_interactive", None)
    name = (di.get("metric") if hasattr(di, "get") else getattr(di, "metric", None)) if di is not None else None
    if name is None:
        raise ValueError("oracle_recommend: cfg.davis_interactive.metric is not set (J, F or J_AND_F)")
    return name


def oracle_recommend(cfg_yl, agent, device, sessions, as_list=False):
    """The oracle setting's interaction tail for several sessions at once: ``misc.sequence_metric`` + ``recommend_frame`` (setting
    "oracle") per session, as ONE device chain.  ``sessions`` is a sequence of dicts with gt_masks, pred_masks ([N,H,W] label maps, numpy
    or device tensors; each session its own length and size), n_objects, annotated_frames_list and prev_frames; the metric is
    cfg.davis_interactive.metric.  Returns (metrics, picks): one numpy float64 [N] array per session - what ``sequence_metric`` returns -
    and the recommended index per session (with ``as_list`` the candidates of ``recommend_candidates``).

    method "ours": one upload of the concatenated annotation counts -> ``metrics.jf_videos`` (one memset and two launches for all
    sessions' counts, one launch for the float64 ratios, the per-frame means and the Brain's fp32 state) -> ``agent.action`` (one
    session) or ``agent.actions`` (several: one ragged Brain forward and one ragged argmax / top-k / spread ranking) -> ONE device-to-host
    copy of [quality (R) float64 | K k indices int64].  agent.candidates, agent.skip_annotated and agent.candidate_gap work as in the
    wild chain of ``recommend_frames``; ``steps_done`` and both host RNG streams move exactly as under sequential ``recommend_frame``
    calls.  method "worst": the quality of the same pass and its one copy, then ``select_next_frame`` / ``worst_candidates`` on the host.
    Metrics and indices equal those of the per-session path bit for bit.  Below ORACLE_MIN_SESSIONS sessions: the per-session path."""
    from . import misc
    from .. import metrics as M
    from ..models.agent import merge_candidates, spread_candidates
    sessions = list(sessions)
    setting, method = cfg_yl.setting, cfg_yl.method
    if setting != "oracle" or method not in ("ours", "worst"):
        raise NotImplementedError(f"oracle_recommend serves setting 'oracle' with method 'ours' or 'worst', got {setting!r} / {method!r}")
    if not sessions:
        return [], []
    name = _oracle_metric_name(cfg_yl)
    k, _, gap = _topk_options(cfg_yl, agent)
    K = len(sessions)
    if K < ORACLE_MIN_SESSIONS:
        out_m, out_p = [], []
        for s in sessions:
            m = misc.sequence_metric(name, s["gt_masks"], s["pred_masks"], s["n_objects"])
            out_m.append(m)
            out_p.append(_recommend_one(cfg_yl, None, agent, device, len(m), s["n_objects"], None, None, m, s["prev_frames"],
                                        s["annotated_frames_list"], None, None, None, k=k, as_list=as_list, gap=gap))
        return out_m, out_p
    ns = [int(s["gt_masks"].shape[0]) for s in sessions]
    R = sum(ns)
    offs = np.concatenate([[0], np.cumsum(ns)])[:-1]
    with torch.no_grad():
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        cnt = None
        if method == "ours":                                              # one upload for all sessions
            cnt = torch.as_tensor(np.concatenate([_annotation_counts(n, s["annotated_frames_list"])
                                                  for n, s in zip(ns, sessions)]).astype(np.float32)).to(dev, non_blocking=True)
        out = torch.zeros(R + K * k, dtype=torch.float64, device=dev)       # [quality of every session (R) | the K k indices (int64 bits)]
        res = M.jf_videos([(s["gt_masks"], s["pred_masks"], s["n_objects"]) for s in sessions], name, annot_counts=cnt, out=out)
        picked = [None] * K
        if method == "ours":
            idx_dev = out[R:].view(torch.int64)
            if K == 1:
                picked = [agent.action(res.state, device_out=idx_dev)]
            else:
                picked = agent.actions([res.state[int(o):int(o) + n] for o, n in zip(offs, ns)], device_out=idx_dev)
        host = out.cpu()                                                    # the one D2H copy of the call
    quality, index = host.numpy(), host.view(torch.int64).numpy()
    out_m, out_p = [], []
    for j, (s, n, o, pk) in enumerate(zip(sessions, ns, offs, picked)):
        m = quality[int(o):int(o) + n].copy()
        out_m.append(m)
        i = R + j * k
        if method == "worst":
            out_p.append(worst_candidates(m, k, s["prev_frames"], gap) if as_list else
                         select_next_frame(m, metric="worst", prev_frames=s["prev_frames"]))
        elif k > 1:                                                         # (a spread ranking is final: the pick is its slot 0 already)
            cand = spread_candidates(index[i:i + k]) if gap > 1 else merge_candidates(pk, index[i:i + k], k)
            out_p.append(cand if as_list else cand[0])
        else:
            pick = pk if pk is not None else np.int64(index[i])
            out_p.append(_candidate_list(pick, 1) if as_list else pick)
    return out_m, out_p
