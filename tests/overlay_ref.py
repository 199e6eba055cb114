"""numpy restatement of the overlay rules of csrc/overlay.hip (include/ivosw.h, "session overlays"): shifted compares, float64 blends
rounded operation by operation, no scipy.  tests/golden/overlay_fixtures.npz pins it to the reference's functions bit for bit
(tests/test_overlay_option.py); the GPU tests compare the kernels with it."""
import numpy as np

STYLES = ("davis", "fade", "checker", "color")


def davis_palette(n=32):
    """The DAVIS / PASCAL-VOC colours of objects 1 .. n, uint8 [n,3]: bit j of the object id feeds bit 7 - j // 3 of channel j % 3."""
    pal = np.zeros((n, 3), np.uint8)
    for o in range(1, n + 1):
        for j in range(24):
            pal[o - 1, j % 3] |= ((o >> j) & 1) << (7 - j // 3)
    return pal


def frame_bytes(frames_f32):
    """The image bytes of float32 frames [n,3,H,W] -> uint8 [n,H,W,3]: rint(f * 255) in float32, clamped to 0 .. 255, NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(frames_f32, np.float32) * np.float32(255.0))
        r = np.where(r >= 0, np.minimum(r, np.float32(255.0)), np.float32(0.0))          # a NaN fails r >= 0
    return np.ascontiguousarray(r.astype(np.uint8).transpose(0, 2, 3, 1))


def effective(label, n_objects, select):
    """The object a label value stands for under ``select``, 0 = none: select = 0 keeps 1 .. n_objects, select = o keeps o alone."""
    label = np.asarray(label).astype(np.int32)
    keep = (label >= 1) & (label <= n_objects) if select == 0 else label == select
    return np.where(keep, label, 0)


def neighbours(e):
    """The four edge neighbours of every pixel of [H,W] (left, right, up, down); 0 outside the image."""
    p = np.pad(e, 1)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def overlay_one(image, label, style, n_objects, select=0, alpha=0.5, palette=None, color=(255, 0, 255)):
    """One picture: image uint8 [H,W,3], label [H,W] -> uint8 [H,W,3]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and style in STYLES
    e = effective(label, n_objects, select)
    nb = neighbours(e)
    inside = e != 0
    near = np.maximum.reduce(nb)
    contour = ~inside & (near != 0)
    out = image.copy()
    if style == "davis":
        palette = davis_palette() if palette is None else np.asarray(palette, np.uint8)
        k = (1.0 * (1 - float(alpha))) * palette.astype(np.float64)                       # [32,3], formed as the reference forms it
        below = np.zeros(e.shape, bool)                                                   # a neighbour of a smaller object: its contour ran first
        for q in nb:
            below |= (q != 0) & (q < e)
        v = np.where(below[..., None], 0.0, image.astype(np.float64))
        prod = v * float(alpha)
        blend = (prod + k[np.maximum(e, 1) - 1]).astype(np.uint8)                         # truncation
        out = np.where(inside[..., None], blend, out)
        out[near > e] = 0                                                                 # the contour of another object ran last (or no own object)
    elif style == "fade":
        out = np.where(inside[..., None], image, (0.4 * image.astype(np.float64)).astype(np.uint8))
        out[contour] = (0, 255, 255)
    elif style == "checker":
        yy, xx = np.mgrid[:e.shape[0], :e.shape[1]]
        board = np.where((yy // 20 + xx // 20) % 2 == 0, 223, 32).astype(np.uint8)
        out = np.where(inside[..., None], image, board[..., None])
    else:
        out = np.where(inside[..., None], image, np.asarray(color, np.uint8)[None, None, :])
    return np.ascontiguousarray(out.astype(np.uint8))


def overlay(images, labels, style, n_objects, frame_ids=None, out="rgb", **kw):
    """images uint8 [n,H,W,3], labels [n,H,W] -> uint8 [m,H,W,3] ("rgb") or [m,H,W,4] with byte 3 = 0 ("rgbx")."""
    ids = range(len(images)) if frame_ids is None else frame_ids
    pics = np.stack([overlay_one(images[f], labels[f], style, n_objects, **kw) for f in ids], 0)
    if out == "rgbx":
        pics = np.concatenate([pics, np.zeros(pics.shape[:3] + (1,), np.uint8)], 3)
    return pics
