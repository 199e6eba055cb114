"""The sampling rule of ivosw_qa_augment (include/ivosw.h, "augmented assessment samples") restated in numpy, written from the header.

Every fp32 operation is one numpy float32 operation, so it is rounded by itself; the device kernel is compiled without FMA contraction
and agrees with this bit for bit.  Sources: ``frames`` float32 [n,3,H,W] or uint8 RGBX [n,H,W,4]; ``gt`` uint8 [n,H,W]; ``planes`` uint8
[O,n,H,W]; ``obj_ids`` a list of O label values.  A map is six numbers a b c d e f: sx = a x + b y + c, sy = d x + e y + f.
"""
import numpy as np

F32 = np.float32
MAX_CAND = 12
IDENTITY = (1., 0., 0., 0., 1., 0.)


def compose(cand, post):
    """The full map of a candidate: post applied to (x, y) first, then the candidate, composed in float64 (each operation rounded by
    itself) and rounded to fp32 once."""
    a, b, c, d, e, f = (np.float64(F32(v)) for v in cand)
    pa, pb, pc, pd, pe, pf = (np.float64(F32(v)) for v in post)
    return np.array([a * pa + b * pd, a * pb + b * pe, (a * pc + b * pf) + c,
                     d * pa + e * pd, d * pb + e * pe, (d * pc + e * pf) + f], dtype=np.float64).astype(F32)


def coords(m, Ho, Wo):
    """sx, sy float32 [Ho,Wo]: fl(fl(fl(a x) + fl(b y)) + c)."""
    m = np.asarray(m, dtype=F32)
    x = np.arange(Wo, dtype=F32)[None, :]
    y = np.arange(Ho, dtype=F32)[:, None]
    with np.errstate(all="ignore"):
        sx = (m[0] * x + m[1] * y) + m[2]
        sy = (m[3] * x + m[4] * y) + m[5]
    return np.broadcast_to(sx, (Ho, Wo)).astype(F32), np.broadcast_to(sy, (Ho, Wo)).astype(F32)


def warp_label(gt, obj_id, m, Ho, Wo):
    """Nearest: the tap (floor(sx + .5), floor(sy + .5)); 0 outside the source, gt == obj_id inside.  uint8 [Ho,Wo]."""
    H, W = gt.shape
    sx, sy = coords(m, Ho, Wo)
    with np.errstate(all="ignore"):
        tx, ty = np.floor(sx + F32(0.5)), np.floor(sy + F32(0.5))
        inside = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    ix = np.where(inside, tx, 0).astype(np.int64)
    iy = np.where(inside, ty, 0).astype(np.int64)
    return (inside & (gt[iy, ix] == obj_id)).astype(np.uint8)


def bilinear(src, m, Ho, Wo):
    """src float32 [H,W] -> float32 [Ho,Wo]; taps outside the source read 0."""
    H, W = src.shape
    sx, sy = coords(m, Ho, Wo)
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = (sx - x0).astype(F32), (sy - y0).astype(F32)

        def tap(dx, dy):
            tx, ty = x0 + F32(dx), y0 + F32(dy)             # (exact: small integers; a far-away value stays outside)
            inside = (x0 >= -dx) & (x0 <= W - 1 - dx) & (y0 >= -dy) & (y0 <= H - 1 - dy)
            ix = np.where(inside, tx, 0).astype(np.int64)
            iy = np.where(inside, ty, 0).astype(np.int64)
            return np.where(inside, src[iy, ix], F32(0)).astype(F32)
        v00, v10, v01, v11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
        top = (v00 + fx * (v10 - v00)).astype(F32)
        bot = (v01 + fx * (v11 - v01)).astype(F32)
        return (top + fy * (bot - top)).astype(F32)


def byte_to_float(b):
    """float32(b) / 255.0f, correctly rounded."""
    return (np.asarray(b).astype(F32) / F32(255.0)).astype(F32)


def photometric(v, noise, contrast):
    with np.errstate(all="ignore"):
        t = np.clip((v + F32(noise)).astype(F32), F32(0), F32(1))
        return np.clip((t * F32(contrast)).astype(F32), F32(0), F32(1)).astype(F32)


def frame_planes(frames, f):
    """The three float32 colour planes [3,H,W] of frame f of either frame kind."""
    if frames.dtype == np.uint8:
        return byte_to_float(np.moveaxis(frames[f, :, :, :3], 2, 0))
    return np.asarray(frames[f], dtype=F32)


def label_flags(gt, obj_id, m, Ho, Wo):
    lab = warp_label(gt, obj_id, m, Ho, Wo)
    return bool((lab == 0).any()), bool((lab == 1).any())


def sample_maps(sample):
    """The maps the kernel sees: one per candidate (composed with post), then post alone."""
    post = np.asarray(sample["post"], dtype=F32)
    return [compose(c, post) for c in sample.get("cands", [])] + [post]


def choose(gt, obj_id, maps, Ho, Wo):
    """The first candidate whose number of distinct label values equals that of "no candidate" (the last map), else their count."""
    n_cand = len(maps) - 1
    if n_cand == 0:
        return 0
    want = sum(label_flags(gt, obj_id, maps[-1], Ho, Wo))
    for c in range(n_cand):
        if sum(label_flags(gt, obj_id, maps[c], Ho, Wo)) == want:
            return c
    return n_cand


def augment(videos, samples, Ho, Wo):
    """videos: [dict(frames, gt, planes, obj_ids)]; samples: [dict(v, f, o, cands=[six numbers, ...], post=six numbers, noise, contrast)].
    Returns dict(img float32 [N,3,Ho,Wo], prob float32 [N,Ho,Wo], label uint8, mask uint8, chosen int32 [N])."""
    N = len(samples)
    img = np.zeros((N, 3, Ho, Wo), F32)
    prob = np.zeros((N, Ho, Wo), F32)
    label = np.zeros((N, Ho, Wo), np.uint8)
    mask = np.zeros((N, Ho, Wo), np.uint8)
    chosen = np.zeros(N, np.int32)
    for k, s in enumerate(samples):
        vid = videos[s["v"]]
        gt, obj_id = vid["gt"][s["f"]], vid["obj_ids"][s["o"]]
        maps = sample_maps(s)
        chosen[k] = choose(gt, obj_id, maps, Ho, Wo)
        m = maps[chosen[k]]
        planes = frame_planes(vid["frames"], s["f"])
        for ch in range(3):
            img[k, ch] = photometric(bilinear(planes[ch], m, Ho, Wo), s.get("noise", 0.), s.get("contrast", 1.))
        prob[k] = bilinear(byte_to_float(vid["planes"][s["o"], s["f"]]), m, Ho, Wo)
        label[k] = warp_label(gt, obj_id, m, Ho, Wo)
        mask[k] = np.where(prob[k] > F32(0.8), 255, 0).astype(np.uint8)
    return dict(img=img, prob=prob, label=label, mask=mask, chosen=chosen)
