"""The train-time augmentations of AssessNet's samples (the reference's datasets/transforms_assess.py) as ONE fused warp on the device.

The reference's seven classes keep their names and constructor signatures, but here a transform *draws parameters* for a batch of device
samples instead of touching pixels: every geometric step is an inverse affine map (destination pixel -> source coordinate), ``Compose``
multiplies the maps of a pipeline in float64 and calls ``ivosw_qa_augment`` ONCE for the whole batch.  The sources (frames, label maps,
byte planes) already live on the device and the outputs stay there; the call does not synchronise.

What is the same as the reference, and what is restated:
  * RandomHorizontalFlip, AdditiveNoise, RandomContrast and RandomCrop take the same draws from the same host streams (``random``,
    ``np.random``) in the same order as the reference's classes: transform by transform, frame (= sample) by frame.
  * imgaug and cv2 are not part of this project's environment.  Parity with their interpolation and border handling, and with imgaug's
    own draw order inside iaa.Crop / iaa.Affine, is restated, not recorded: the sampling rule of include/ivosw.h is the definition
    (bilinear with zero outside, nearest for the label, pixel-centre resizing).
  * RandomAffine draws its 12 seeds per frame up front (``random.randint(0, 2020)`` twelve times), where the reference draws one seed per
    retry and stops at the first that keeps the number of label values; the device then picks the first candidate that does.  The host
    streams therefore advance by 12 draws per frame whatever the labels hold - the price of never reading the labels back.
"""
import math
import random

import numpy as np
import torch

from .. import _lib as L

N_TRIES = L.QA_AUG_MAX_CAND          # the reference's retry loop gives up after 12 tries (timing > 10)


def _mat(a, b, c, d, e, f):
    return np.array([[a, b, c], [d, e, f], [0., 0., 1.]], dtype=np.float64)


def resize_map(W, H, Wo, Ho):
    """Inverse map of a resize from W x H to Wo x Ho by pixel centres: sx = (x + .5) * W / Wo - .5 (the identity at equal sizes)."""
    kx, ky = W / Wo, H / Ho
    return _mat(kx, 0., 0.5 * kx - 0.5, 0., ky, 0.5 * ky - 0.5)


def flip_map(W):
    return _mat(-1., 0., W - 1., 0., 1., 0.)


def crop_map(x0, y0):
    return _mat(1., 0., float(x0), 0., 1., float(y0))


def affine_inverse(W, H, crop, scale, shear, rotate):
    """Inverse map of the reference's iaa.Crop(keep_size) + iaa.Affine pair on a W x H frame, as restated here.
    Forward: crop ``crop`` = (top, right, bottom, left) fractions of H / W off the borders, resize the rectangle back to W x H by pixel
    centres, then about the centre ((W - 1) / 2, (H - 1) / 2): scale, x-shear by ``shear`` degrees ([[1, tan], [0, 1]]), rotation by
    ``rotate`` degrees ([[cos, -sin], [sin, cos]]).  Returns the float64 3 x 3 matrix destination -> source."""
    top, right, bottom, left = (float(v) for v in crop)
    t, b, l, r = top * H, bottom * H, left * W, right * W
    kx, ky = (W - l - r) / W, (H - t - b) / H
    crop_inv = _mat(kx, 0., 0.5 * kx - 0.5 + l, 0., ky, 0.5 * ky - 0.5 + t)
    cx, cy = (W - 1) / 2., (H - 1) / 2.
    th, ph = math.radians(rotate), math.radians(shear)
    rot = _mat(math.cos(th), -math.sin(th), 0., math.sin(th), math.cos(th), 0.)
    shx = _mat(1., math.tan(ph), 0., 0., 1., 0.)
    scl = _mat(scale, 0., 0., 0., scale, 0.)
    fwd = _mat(1., 0., cx, 0., 1., cy) @ rot @ shx @ scl @ _mat(1., 0., -cx, 0., 1., -cy)
    return crop_inv @ np.linalg.inv(fwd)


class _Geometric:
    """A transform that changes where pixels come from: ``draw(sizes)`` -> (one inverse 3 x 3 float64 matrix per sample - or, for
    RandomAffine, a list of candidates per sample - and the sizes [(W, H)] after the transform)."""
    candidates = False


class Resize(_Geometric):
    """Resize every frame to ``size`` = (W, H) by pixel centres (the reference's three cv2.resize calls; ``scales`` is unused there too)."""

    def __init__(self, scales=[0.5, 0.8, 1], size=(854, 480)):
        self.scales = scales
        self.size = size

    def draw(self, sizes):
        Wo, Ho = int(self.size[0]), int(self.size[1])
        return [resize_map(W, H, Wo, Ho) for W, H in sizes], [(Wo, Ho)] * len(sizes)


class RandomHorizontalFlip(_Geometric):
    """Horizontally flip each frame with a probability of 0.5: ``random.random() < 0.5`` per frame, the map a = -1, c = W - 1."""

    def draw(self, sizes):
        return [flip_map(W) if random.random() < 0.5 else np.eye(3) for W, H in sizes], list(sizes)


class ToTensor:
    """The outputs of the device warp are tensors in AssessNet's layout already: kept for the reference's pipelines, does nothing."""


class RandomAffine(_Geometric):
    """Affine transformation of each frame: 12 candidate maps per frame, of which the device takes the first that keeps the number of
    label values (the reference's retry loop, see the module's header).  Per frame 12 seeds ``random.randint(0, 2020)`` are drawn up
    front; from ``np.random.RandomState(seed)`` come, in this order: the four crop fractions (top, right, bottom, left) uniform in
    (0, 0.1), the scale in (0.9, 1.1), the x-shear in (-15, 15) degrees, the rotation in (-25, 25) degrees (``affine_inverse``)."""
    candidates = True

    @staticmethod
    def params(seed):
        rs = np.random.RandomState(seed)
        crop = rs.uniform(0.0, 0.1, 4)
        return crop, rs.uniform(0.9, 1.1), rs.uniform(-15., 15.), rs.uniform(-25., 25.)

    def draw(self, sizes):
        out = []
        for W, H in sizes:
            seeds = [random.randint(0, 2020) for _ in range(N_TRIES)]
            out.append([affine_inverse(W, H, *self.params(s)) for s in seeds])
        return out, list(sizes)


class AdditiveNoise:
    """One value ``np.random.uniform(-delta / 255, delta / 255)`` per frame, added to the warped image and clipped to 0 .. 1."""

    def __init__(self, delta=5.0):
        self.delta = delta
        assert delta > 0.0

    def draw(self, n):
        return [np.random.uniform(-self.delta / 255., self.delta / 255.) for _ in range(n)]


class RandomContrast:
    """One factor ``np.random.uniform(lower, upper)`` per frame, multiplied into the image and clipped to 0 .. 1."""

    def __init__(self, lower=0.97, upper=1.03):
        self.lower = lower
        self.upper = upper
        assert self.lower <= self.upper
        assert self.lower > 0

    def draw(self, n):
        return [np.random.uniform(self.lower, self.upper) for _ in range(n)]


class RandomCrop(_Geometric):
    """A random ``patch_size`` square of each frame: ``random.randint(0, H - patch_size)`` then ``random.randint(0, W - patch_size)``.
    The reference draws again (up to 12 times) until the patch's label holds the background and something else, and renumbers the label
    values; that rule needs the label's values on the host, so here the crop stays a SINGLE draw per frame and the label is the
    object's 0 / 1 mask as everywhere in this module."""

    def __init__(self, patch_size=400):
        self.patch_size = patch_size

    def draw(self, sizes):
        maps = []
        for W, H in sizes:
            assert min(W, H) > self.patch_size
            h_start = random.randint(0, H - self.patch_size)
            w_start = random.randint(0, W - self.patch_size)
            maps.append(crop_map(w_start, h_start))
        return maps, [(self.patch_size, self.patch_size)] * len(sizes)


class DeviceSamples:
    """The sources of a batch on the device plus its sample list.  ``videos``: [(frames, gt, planes[, obj_ids]), ...] with frames a float32
    device tensor [n,3,H,W] or a PackedFrames (RGBX8), gt uint8 [n,H,W], planes uint8 [O,n,H,W] (``metrics.quantize_probs``), obj_ids the
    label value of each plane (default 1 .. O).  ``samples``: [(video, frame, object index), ...]."""

    def __init__(self, videos, samples):
        self.videos, self.samples, self._keep = [], [(int(v), int(f), int(o)) for v, f, o in samples], []
        if not videos or len(videos) > L.MAX_JF_VIDEOS:
            raise ValueError(f"DeviceSamples takes 1 .. {L.MAX_JF_VIDEOS} videos, got {len(videos)}")
        if not self.samples:
            raise ValueError("DeviceSamples needs at least one sample")
        self.device = None
        for i, video in enumerate(videos):
            frames, gt, planes = video[:3]
            packed = hasattr(frames, "rgbx")
            fr = frames.rgbx if packed else frames
            for name, t, dt in (("frames", fr, torch.uint8 if packed else torch.float32), ("gt", gt, torch.uint8), ("planes", planes, torch.uint8)):
                L.dptr(t, dt)                                      # device, dtype, contiguous: no CPU fallback
            n, H, W = (int(d) for d in gt.shape)
            O = int(planes.shape[0])
            want = (n, H, W, 4) if packed else (n, 3, H, W)
            if tuple(fr.shape) != want or tuple(planes.shape) != (O, n, H, W):
                raise ValueError(f"video {i}: frames {tuple(fr.shape)} / planes {tuple(planes.shape)} do not match the label map {tuple(gt.shape)}")
            ids = list(video[3]) if len(video) > 3 and video[3] is not None else list(range(1, O + 1))
            if len(ids) != O or not 1 <= O <= 32:
                raise ValueError(f"video {i}: 1 .. 32 planes with one object id each")
            d = L.AugVideo(frames=fr.data_ptr(), gt=gt.data_ptr(), planes=planes.data_ptr(),
                           frames_kind=L.FRAMES_RGBX8 if packed else L.FRAMES_F32, n_frames=n, H=H, W=W, n_obj=O)
            for k, v in enumerate(ids):
                d.obj_ids[k] = int(v)
            self.videos.append(d)
            self._keep.append((fr, gt, planes))
            self.device = gt.device
        self.table = (L.AugVideo * len(self.videos))(*self.videos)

    def sizes(self):
        return [(self.videos[v].W, self.videos[v].H) for v, f, o in self.samples]

    def __len__(self):
        return len(self.samples)


_ws = {}      # (device index, stream handle) -> flag workspace: calls on different streams of one device never share the flag bytes


def _six(m):
    return [float(m[0, 0]), float(m[0, 1]), float(m[0, 2]), float(m[1, 0]), float(m[1, 1]), float(m[1, 2])]


def sample_table(ds, rows):
    """The host array of ivosw_qa_aug_sample_t rows for ``ds`` from ``rows`` = one dict(cands=[six numbers, ...], post=six numbers, noise,
    contrast) per sample (absent: no candidate, the identity, 0, 1).  Returns (table, whether any sample has a candidate)."""
    N = len(ds)
    if len(rows) != N:
        raise ValueError(f"{len(rows)} parameter rows for {N} samples")
    table = (L.AugSample * N)()
    any_cand = False
    for k, ((v, f, o), row) in enumerate(zip(ds.samples, rows)):
        s = table[k]
        s.v, s.f, s.o = v, f, o
        cands = row.get("cands", [])
        if len(cands) > L.QA_AUG_MAX_CAND:
            raise ValueError(f"sample {k}: {len(cands)} candidates, at most {L.QA_AUG_MAX_CAND}")
        s.n_cand = len(cands)
        any_cand = any_cand or len(cands) > 0
        for c, m in enumerate(cands):
            s.cand[c] = (L.C.c_float * 6)(*m)
        s.post = (L.C.c_float * 6)(*row.get("post", (1., 0., 0., 0., 1., 0.)))
        s.noise, s.contrast = row.get("noise", 0.), row.get("contrast", 1.)
    return table, any_cand


def empty_outputs(N, Ho, Wo, dev):
    return dict(img=torch.empty((N, 3, Ho, Wo), dtype=torch.float32, device=dev), prob=torch.empty((N, Ho, Wo), dtype=torch.float32, device=dev),
                label=torch.empty((N, Ho, Wo), dtype=torch.uint8, device=dev), mask=torch.empty((N, Ho, Wo), dtype=torch.uint8, device=dev),
                chosen=torch.empty(N, dtype=torch.int32, device=dev))


def workspace(N, dev):
    """A uint8 device tensor of ivosw_qa_augment_ws_bytes(N) for the candidate flags, for a caller that owns its workspace (graph capture)."""
    return torch.empty(max(int(L.lib().ivosw_qa_augment_ws_bytes(N)), 1), dtype=torch.uint8, device=dev)


def launch(ds, table, any_cand, Ho, Wo, out, ws=None):
    """The C call alone: ``table`` from ``sample_table``, ``out`` from ``empty_outputs``.  ``ws``: the caller's flag workspace; None takes
    one cached per (device, current stream), allocated at the first call on that stream - inside a graph capture hand one in."""
    N, dev = len(ds), ds.device
    lib = L.lib()
    if any_cand and ws is None:
        nbytes = int(lib.ivosw_qa_augment_ws_bytes(N))
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = _ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _ws[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    use_ws = any_cand and ws is not None
    L.check(lib.ivosw_qa_augment(ds.table, len(ds.videos), table, N, int(Ho), int(Wo), L.dptr(out["img"], torch.float32),
                                 L.dptr(out["prob"], torch.float32), L.dptr(out["label"], torch.uint8), L.dptr(out["mask"], torch.uint8),
                                 L.dptr(out["chosen"], torch.int32), L.dptr(ws, torch.uint8) if use_ws else None,
                                 ws.numel() if use_ws else 0, L.stream_ptr(dev)), "qa_augment")
    return out


def augment(ds, rows, Ho, Wo, out=None, ws=None):
    """``ivosw_qa_augment`` on a DeviceSamples: ``rows`` as ``sample_table`` takes them.  Returns dict(img, prob, label, mask, chosen) of
    device tensors (``out`` / ``ws``: preallocated outputs and flag workspace, for graph capture); no synchronisation."""
    table, any_cand = sample_table(ds, rows)
    return launch(ds, table, any_cand, Ho, Wo, empty_outputs(len(ds), Ho, Wo, ds.device) if out is None else out, ws)


class Compose:
    """A pipeline of the transforms above.  ``draw(sizes)`` takes every transform's draws in pipeline order (transform by transform, sample
    by sample, as the reference's loops do) and composes the inverse maps in float64; ``__call__(device_samples)`` runs the ONE device
    call and returns dict(img, prob, label, mask, chosen) of device tensors without synchronising.
    With P the product of the maps before RandomAffine, A a candidate and Q the product of those after it, the sample's map is P A Q;
    the device composes candidate-after-post, so it is handed post = P Q and candidate = P A P^-1 (their product is P A Q, and "no
    candidate" is P Q: the untransformed sample still passes through Resize and the flip).  AdditiveNoise must come before
    RandomContrast (the kernel's order, the reference's too); both act on the warped image."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        kinds = [type(t) for t in self.transforms]
        if sum(k is RandomAffine for k in kinds) > 1:
            raise ValueError("Compose: at most one RandomAffine (one set of candidates per sample)")
        if sum(k is AdditiveNoise for k in kinds) > 1 or sum(k is RandomContrast for k in kinds) > 1:
            raise ValueError("Compose: at most one AdditiveNoise and one RandomContrast")
        if AdditiveNoise in kinds and RandomContrast in kinds and kinds.index(RandomContrast) < kinds.index(AdditiveNoise):
            raise ValueError("Compose: AdditiveNoise comes before RandomContrast (the order the device applies them in)")

    def draw(self, sizes):
        """-> (rows for ``augment``, (Wo, Ho)); every sample must end at the same size."""
        n = len(sizes)
        pre, post, cands = [np.eye(3) for _ in range(n)], [np.eye(3) for _ in range(n)], None
        noise, contrast = [0.] * n, [1.] * n
        for t in self.transforms:
            if isinstance(t, AdditiveNoise):
                noise = t.draw(n)
            elif isinstance(t, RandomContrast):
                contrast = t.draw(n)
            elif isinstance(t, _Geometric):
                maps, sizes = t.draw(sizes)
                if t.candidates:
                    cands = maps
                elif cands is None:
                    pre = [p @ m for p, m in zip(pre, maps)]
                else:
                    post = [q @ m for q, m in zip(post, maps)]
            elif not isinstance(t, ToTensor):
                raise TypeError(f"Compose: {type(t).__name__} is not a transform of this module")
        if len(set(sizes)) != 1:
            raise ValueError(f"Compose: the samples end at different sizes {sorted(set(sizes))}: add a Resize or a RandomCrop")
        rows = []
        for k in range(n):
            row = dict(post=_six(pre[k] @ post[k]), noise=noise[k], contrast=contrast[k])
            if cands is not None:
                inv = np.linalg.inv(pre[k])
                row["cands"] = [_six(pre[k] @ a @ inv) for a in cands[k]]
            rows.append(row)
        return rows, sizes[0]

    def __call__(self, device_samples):
        rows, (Wo, Ho) = self.draw(device_samples.sizes())
        return augment(device_samples, rows, Ho, Wo)


def train_transform(size=(854, 480)):
    """The reference's train pipeline (quality_assessment.py): Resize, RandomAffine, AdditiveNoise, RandomContrast, RandomHorizontalFlip."""
    return Compose([Resize(size=size), RandomAffine(), AdditiveNoise(), RandomContrast(), RandomHorizontalFlip(), ToTensor()])
