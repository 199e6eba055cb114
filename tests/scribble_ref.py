"""The numpy DEFINITION of the scribble rasteriser (csrc/scribble.hip, utils/scribbles.py): packing, the sequential line loop, the order
of assignment, and the rough_ROI rule written from its statement in include/ivosw.h (not copied from the reference: the reference's own
function is recorded in tests/golden/scribble_fixtures.npz and compared with this one on the CPU).

davisinteractive's scribbles2mask is not in the reference tree and the package is not installed where this was written, so parity with
the library's rasteriser is restated here, not recorded."""
import numpy as np


def pack_point(x, y, H, W):
    """(px, py): the float64 products truncated, 1.0 clamped to the last pixel."""
    return min(int(np.float64(x) * W), W - 1), min(int(np.float64(y) * H), H - 1)


def line_loop(x0, y0, x1, y1):
    """The pixels of (x0,y0) -> (x1,y1), in plot order: the sequential loop that IS the line rule."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x1 - x0 > 0 else -1
    sy = 1 if y1 - y0 > 0 else -1
    xdrive = dx > dy                                       # dx == dy: y drives
    a, b = (dx, dy) if xdrive else (dy, dx)
    D, m, out = 2 * b - a, 0, []
    for s in range(a + 1):
        out.append((x0 + sx * s, y0 + sy * m) if xdrive else (x0 + sx * m, y0 + sy * s))
        if D >= 0:
            m += 1
            D -= 2 * a
        D += 2 * b
    return out


def minor_loop(a, b):
    """m at every step s = 0 .. a of the loop above (b <= a)."""
    D, m, out = 2 * b - a, 0, []
    for _ in range(a + 1):
        out.append(m)
        if D >= 0:
            m += 1
            D -= 2 * a
        D += 2 * b
    return out


def minor_closed(a, b, s):
    """The closed form the kernel uses, a > 0."""
    return (2 * b * s + a) // (2 * a)


def draw_paths(mask, paths, bresenham=True):
    """``paths``: a list of (integer points [[px, py], ...], object id) drawn into ``mask`` [H,W] in list order, later over earlier."""
    for pts, obj in paths:
        pts = [(int(p[0]), int(p[1])) for p in pts]
        if not pts:
            continue
        if not bresenham or len(pts) == 1:
            pix = pts
        else:
            pix = [q for (p0, p1) in zip(pts[:-1], pts[1:]) for q in line_loop(p0[0], p0[1], p1[0], p1[1])]
        for x, y in pix:
            mask[y, x] = obj
    return mask


def raster(points, table, n_maps, H, W, default_value=-1, bresenham=True):
    """What ivosw_scribble_raster draws from a packed (points [P,2], table [n_paths,4]) pair: int8 [n_maps,H,W]."""
    out = np.full((n_maps, H, W), default_value, np.int8)
    for first, n, obj, m in np.asarray(table).reshape(-1, 4):
        draw_paths(out[m], [(np.asarray(points)[first:first + n], obj)], bresenham)
    return out


def scribbles2mask(scribbles, size, bresenham=True, default_value=-1, dtype=np.int8):
    """All frames of a davisinteractive-schema dict at ``size`` = (H, W): [n_frames,H,W] (``dtype`` int64 is what the library allocates)."""
    H, W = size
    per_frame = scribbles["scribbles"]
    out = np.full((len(per_frame), H, W), default_value, dtype)
    for f, paths in enumerate(per_frame):
        draw_paths(out[f], [([pack_point(x, y, H, W) for x, y in p["path"]], p["object_id"]) for p in paths], bresenham)
    return out


def rough_roi(labels, dist=20):
    """[b,1,h,w] -> the same shape: per image the box of the pixels != -1 (a NaN is != -1); rows [max(hmin - dist, 0), min(hmax + dist,
    h - 1)) x columns [max(wmin - dist, 0), min(wmax + dist, w - 1)) keep their value, the rest is 0; an image without such a pixel is
    all 0 (the one stated difference from the reference, which raises)."""
    labels = np.asarray(labels)
    b, _, h, w = labels.shape
    out = np.zeros_like(labels)
    for i in range(b):
        ys, xs = np.nonzero(labels[i, 0] != -1)
        if ys.size == 0:
            continue
        r0, r1 = max(int(ys.min()) - dist, 0), min(int(ys.max()) + dist, h - 1)
        c0, c1 = max(int(xs.min()) - dist, 0), min(int(xs.max()) + dist, w - 1)
        out[i, 0, r0:r1, c0:c1] = labels[i, 0, r0:r1, c0:c1]
    return out
