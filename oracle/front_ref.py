"""ORACLE (test infrastructure — never imported by the product path).

float64 references of the small kernels around the conv tower, and the test inputs and the error bound that the CPU test
(tests/test_oracle_front.py) and the GPU test (tests/test_gpu_front_edges.py) share:

  * ``bbox_ref``       (tp > 0.5) on the raw float32 plane (NaN = background), then assess_oracle.mask_bbox_yxhw
  * ``roi_points64``   the 256 + 256 source coordinates of a ROI tile: roi_theta, the linspace and roi_sample of
                       assess_oracle evaluated in float64 from the float32 box values, linspace exactly -1 + 2 i / 255
  * ``roi_sample64``   bilinear, zero padding, align_corners=True on those points, float64 throughout
  * ``lipschitz`` / ``lipschitz_interior``   largest neighbour difference of an image along x and along y
  * ``roi_bound``      the per-value error bound of a fp32 ROI sampler against ``roi_sample64`` (derivation in its docstring)
  * ``quality_ref``    pred.mean(1) of the reference's float64 [n_frames, n_obj] array (numpy's own summation order)
  * ``head_ref``       float64 mean over the 8 x 8 positions, float64 dot product with fc1

and, for the table-driven front end (tests/test_oracle_front_multi.py, tests/test_gpu_front_multi_edges.py):

  * ``scan_seams_multi`` / ``scan_edges``   the chunk of a launch over a video table and the flat indices at which a lone pixel
                       shows a wrong chunk seam, stride or last vector (float4 scan and 16-byte label scan)
  * ``scan_walk``      the kernel's carried (y, x) walk, with switches for two deliberately wrong scans
  * ``label_planes`` / ``label_delta_ref``   the one-hot planes of a label map in unit order, and the dirty units between two maps
  * ``hard_byte_map``  label bytes next to the values a sloppy zero-byte test confuses them with

Plain numpy; imports nothing from the product.
"""
import numpy as np

from oracle import assess_oracle as ao

MEAN = np.array([0.485, 0.456, 0.406], np.float64)
STD = np.array([0.229, 0.224, 0.225], np.float64)
EPS32 = 2.0 ** -24          # unit roundoff of float32


# ---------------------------------------------------------------- mask -> box
def bbox_ref(tp):
    """tp [B,H,W] float32, any values -> [B,4] float32 (y,x,h,w)."""
    tp = np.asarray(tp, np.float32)
    return ao.mask_bbox_yxhw((tp > np.float32(0.5)).astype(np.float32), 1.5)       # NaN > 0.5 is False


def bbox_minmax_ref(tp):
    """The integer box before the growth and clamp rules: int32 [B,4] (ymin, ymax, xmin, xmax), (INT_MAX, -1, INT_MAX, -1) for an
    empty plane - what the scan leaves in ivosw_mask_bbox's scratch.  On frames below ~ 60 pixels every box grows to the 128-pixel
    minimum and is clamped to the whole frame, so the (y,x,h,w) rows alone cannot tell a wrong coordinate there; these can."""
    fg = np.asarray(tp, np.float32) > np.float32(0.5)
    big = np.iinfo(np.int32).max
    out = np.empty((fg.shape[0], 4), np.int32)
    for b in range(fg.shape[0]):
        rows, cols = np.flatnonzero(fg[b].any(1)), np.flatnonzero(fg[b].any(0))
        out[b] = (big, -1, big, -1) if rows.size == 0 else (rows[0], rows[-1], cols[0], cols[-1])
    return out


def scan_seams(B, H, W):
    """Flat indices at which one scan workgroup's range ends and the next begins, from the rule documented in launch_mask_bbox:
    S = clamp(2048 / B, 1, 64) workgroups per plane, each a chunk of ceil(plane / S) elements rounded up to 1024."""
    plane = H * W
    S = max(1, min(64, 2048 // B))
    chunk = -(-plane // S)
    chunk = -(-chunk // 1024) * 1024
    return list(range(chunk, plane, chunk))


BBOX_SIZES = ((480, 854), (37, 53), (5, 3), (4, 3), (8, 2), (16, 1), (1, 16), (1, 1), (2, 2), (3, 1100), (4, 1024), (4, 1025),
              (130, 8), (129, 131))


def threshold_values():
    half = np.float32(0.5)
    return np.array([half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), 0.49, -1.0, np.nan, np.inf], np.float32)


def sparse_plane(rs, H, W):
    """A few foreground pixels (0.9) on a background of 0 .. 0.1."""
    p = min(1.0, max(0.002, 3.0 / (H * W)))
    return np.where(rs.rand(H, W) < p, 0.9, 0.1 * rs.rand(H, W)).astype(np.float32)


def bbox_planes(H, W):
    """One batch [B,H,W] float32 of the planes at which a min/max scan goes wrong, and the seams of THAT batch size: empty, full,
    one pixel at each corner, at flat index H*W - 1 and H*W - 4, a row stripe, a column stripe, blobs whose last - first row and
    column is 126 .. 129 (both sides of the `< 128` growth rule, as rows - 1 and as rows) where the size allows, planes of values
    around the threshold, random sparse planes, and one pixel on each side of every seam between two scan workgroups.  The seams
    depend on B and B on the number of seams: B is the smallest batch that holds them all (spare slots take sparse planes)."""
    rs = np.random.RandomState(H * 10007 + W)
    plane = H * W
    one = lambda i: (np.arange(plane) == i).astype(np.float32).reshape(H, W)        # noqa: E731
    ps = [np.zeros((H, W), np.float32), np.ones((H, W), np.float32)]
    ps += [one(i) for i in (0, W - 1, plane - W, plane - 1)]                        # the four corners
    ps += [one(plane - 1)] + ([one(plane - 4)] if plane >= 4 else [])
    row, col = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    row[H // 2, :] = 1
    col[:, W // 2] = 1
    ps += [row, col]
    for d in (126, 127, 128, 129):
        if H <= d and W <= d:
            continue
        b = np.zeros((H, W), np.float32)
        ys = slice(min(2, H - 1 - d), min(2, H - 1 - d) + d + 1) if H > d else slice(H // 3, H // 3 + 1)
        xs = slice(min(3, W - 1 - d), min(3, W - 1 - d) + d + 1) if W > d else slice(W // 3, W // 3 + 1)
        b[ys, xs] = 0.75
        ps.append(b)
    # around the threshold: a plane of ONE background value (0.5 itself, the float below it, 0.49, -1, NaN) with the values above the
    # threshold (the float above 0.5, +inf) confined to an inner rectangle - a scan that takes that background value for foreground
    # grows the box to the whole plane - and one plane of all seven values mixed
    tv = threshold_values()
    ys, xs = slice(H // 4, max(H // 4 + 1, 3 * H // 4)), slice(W // 4, max(W // 4 + 1, 3 * W // 4))
    for v in tv[[0, 2, 3, 4, 5]]:
        b = np.full((H, W), v, np.float32)
        if plane > 1:
            b[ys, xs] = rs.choice(tv[[1, 6]], size=b[ys, xs].shape)
            b[ys.start, xs.start], b[ys.stop - 1, xs.stop - 1] = tv[1], tv[6]
        ps.append(b)
    ps.append(rs.choice(tv, size=(H, W)))
    ps.append(sparse_plane(rs, H, W))
    B = len(ps)
    while len(ps) + 2 * len(scan_seams(B, H, W)) > B:
        B += 1
    seams = scan_seams(B, H, W)
    for s in seams:
        ps += [one(s - 1), one(s)]
    ps += [sparse_plane(rs, H, W) for _ in range(B - len(ps))]
    assert len(ps) == B and scan_seams(B, H, W) == seams
    return np.stack(ps).astype(np.float32), seams


def stride_edges(H, W, stride=1024, vec=4):
    """Flat indices on each side of every 1024-element stride of the float4 scan (a workgroup of 256 lanes x 4 elements advances
    by 1024 and carries (y, x) across), plus the plane's first and last pixels, its last vector and the ends of the first and last
    row.  ``stride=4096, vec=16``: the same for the 16-pixel byte vectors of the label scan."""
    plane = H * W
    pos = {0, W - 1, plane - W, plane - 1, max(0, plane - vec)}
    for s in range(stride, plane, stride):
        pos |= {s - 1, s, min(plane - 1, s + vec - 1)}
    return sorted(pos)


# ---------------------------------------------------------------- mask -> box over a video table (units, label maps)
def scan_seams_multi(planes, B):
    """The rule of launch_mask_bbox_multi restated: a launch over B unit rows whose videos' planes hold ``planes`` elements asks for
    S = max(1, min(64, 2048 // B)) workgroups per row, cuts the LARGEST plane into chunks of ceil(max(planes) / S) elements rounded up
    to 1024 and recomputes S from that chunk; every video is cut at the same chunk, and a workgroup that starts behind a smaller
    plane leaves.  -> (chunk, [the seams inside plane p for p in planes])."""
    planes = [int(p) for p in planes]
    big = max(planes)
    S = max(1, min(64, 2048 // int(B)))
    chunk = -(-big // S)
    chunk = -(-chunk // 1024) * 1024
    S = -(-big // chunk)
    seams = [list(range(chunk, p, chunk)) for p in planes]
    assert max(len(s) for s in seams) == S - 1
    return chunk, seams


def scan_edges(H, W, chunk, stride=1024, vec=4):
    """Where a lone pixel shows a wrong chunked vector scan of an H x W plane (``stride`` = 1024 elements and ``vec`` = 4 for the float
    scan, 4096 and 16 for the label scan): both sides of every seam between two chunks, both sides of every stride a workgroup takes
    INSIDE its chunk (counted from the chunk's start: 7168 is no multiple of 4096) with the last element of the vector that starts
    there, the plane's first and last element, the first element of its last vector and the ends of the first and last row."""
    plane = H * W
    pos = {0, W - 1, plane - W, plane - 1, max(0, plane - vec)}
    for beg in range(0, plane, chunk):
        if beg:
            pos |= {beg - 1, beg}
        for s in range(beg + stride, min(plane, beg + chunk), stride):
            pos |= {s - 1, s, min(plane - 1, s + vec - 1)}
    return sorted(pos)


def lone_positions(H, W, B, label=False, strides=True):
    """(chunk, scan_edges) of ONE H x W plane scanned in a launch of B rows; ``strides=False`` leaves the strides inside a chunk out
    (480 x 854 at S = 64 has 58 x 6 of them: the carried step there is already used by the pixel before every seam)."""
    chunk, _ = scan_seams_multi([H * W], B)
    stride, vec = (4096, 16) if label else (1024, 4)
    return chunk, scan_edges(H, W, chunk, stride if strides else chunk, vec)


def scan_walk(p, H, W, chunk, stride=1024, vec=4, wrap=True, drop_last=False):
    """The (y, x) at which the vector scan of bbox_scan_multi_kernel meets flat index p, by the kernel's own walk: the lane's first
    vector of the chunk gets its coordinates from a division, every later visit from the carried step (sy, sx) = divmod(stride, W)
    with one row wrap, and the elements inside a vector count on with a wrap each.  Equal to divmod(p, W) when the walk is right.
    The two switches build the WRONG scans that the lone-pixel inputs have to tell from the right one: ``wrap=False`` forgets the row
    wrap of the carried step, ``drop_last=True`` never visits the last vector of a chunk (-> None)."""
    plane = H * W
    beg = p // chunk * chunk
    end = min(plane, beg + chunk)
    o = p - beg
    if drop_last and o >= (end - beg) - vec:
        return None
    first = beg + o % stride // vec * vec
    y, x = divmod(first, W)
    sy, sx = divmod(stride, W)
    for _ in range(o // stride):
        y, x = y + sy, x + sx
        if wrap and x >= W:
            y, x = y + 1, x - W
    for _ in range(o % vec):
        x += 1
        if x == W:
            y, x = y + 1, 0
    return y, x


def label_planes(lab, n_obj):
    """lab [n_frames,H,W] uint8 -> the one-hot planes of include/ivosw.h in unit order, float32 [n_obj * n_frames, H, W]: the plane of
    unit obj * n_frames + frame is (lab[frame] == obj + 1) ? 1 : 0.  The box reference of a label video is bbox_ref / bbox_minmax_ref
    on these planes."""
    lab = np.asarray(lab, np.uint8)
    return np.concatenate([(lab == o + 1).astype(np.float32) for o in range(n_obj)], 0)


def label_delta_ref(old, new, n_obj):
    """old, new [n_frames,H,W] uint8 -> the dirty units of ivosw_mask_delta_videos_lab on a warm video, ascending, numbered inside the
    video (obj * n_frames + frame): a byte going a -> b dirties (frame, a - 1) and (frame, b - 1) when those labels lie in 1 .. n_obj."""
    old, new = np.asarray(old, np.uint8), np.asarray(new, np.uint8)
    n_frames = old.shape[0]
    f = np.nonzero(old != new)[0]
    dirty = set()
    for lab in (old[old != new], new[old != new]):
        ok = (lab >= 1) & (lab <= n_obj)
        dirty |= set(((lab[ok].astype(np.int64) - 1) * n_frames + f[ok]).tolist())
    return sorted(dirty)


MULTI_CARRY_SIZES = ((70, 1100), (80, 1024))                     # chunk 2048 at B <= 32: the second visit is carried (sy = 0 / sx = 0)
ONE_CHUNK_SIZES = ((4, 1025), (4, 1024), (4, 1100), (2048, 2), (8, 8))
LABEL_ONE_CHUNK_SIZES = ((16, 1100), (16, 1024))


def hard_bytes(label):
    """Twelve bytes around ``label`` for a zero-byte test on word ^ label: two words that hold the label next to label ^ 0x80,
    label - 1, label + 1, 0 and 255, and one that holds only those neighbours (for label 255 the 255 is left out)."""
    lo, hi, fl, top = (label - 1) & 255, (label + 1) & 255, label ^ 0x80, 255 if label != 255 else 0
    return np.array([fl, label, lo, hi, label, 0, top, fl, fl, lo, hi, top], np.uint8)


def hard_byte_map():
    """uint8 [5,16,256] for n_obj = 255: label L's twelve hard_bytes sit in the 16-byte vector at flat index 16 * L (at a word offset
    that alternates), on a background of 0.  Frame 0 holds the even labels below 128, frame 1 the odd ones, frames 2 and 3 the same
    above 127 - so no frame holds a label together with label - 1, label + 1 or label ^ 0x80 as labels of their own, and the plane of
    a frame's own label is exactly its two bytes (255 alone is everybody's neighbour: frame 4 holds only its block)."""
    m = np.zeros((5, 16 * 256), np.uint8)
    for lab in range(1, 256):
        f = 4 if lab == 255 else 2 * (lab >> 7) + (lab & 1)
        at = 16 * lab + 4 * ((lab >> 1) & 1)
        m[f, at:at + 12] = hard_bytes(lab)
    return m.reshape(5, 16, 256)


def hard_byte_units(n_obj=255):
    """(frame, label) of the hard_byte_map units whose plane is exactly the label's own two bytes."""
    return [(4 if lab == 255 else 2 * (lab >> 7) + (lab & 1), lab) for lab in range(1, n_obj + 1)]


def lone_planes(H, W, positions):
    """float32 [len(positions), H, W]: plane k is zero but for a 1 at flat index positions[k]."""
    out = np.zeros((len(positions), H * W), np.float32)
    out[np.arange(len(positions)), np.asarray(positions, np.int64)] = 1.0
    return out.reshape(-1, H, W)


def lone_label_map(H, W, positions):
    """uint8 [H, W] (up to 255 positions): label k + 1 at flat index positions[k] and nowhere else, 0 around - the one-hot plane of
    object k is lone_planes' plane k."""
    assert len(positions) <= 255 and len(set(positions)) == len(positions)
    out = np.zeros(H * W, np.uint8)
    out[np.asarray(positions, np.int64)] = np.arange(1, len(positions) + 1)
    return out.reshape(H, W)


# ---------------------------------------------------------------- ROI sampler
def roi_points64(yxhw_f32, H, W):
    """[B,4] float32 boxes -> (sx [B,256], sy [B,256]) float64 pixel coordinates of the output columns / rows."""
    r = np.asarray(np.asarray(yxhw_f32, np.float32), np.float64)
    ymin, ymax = r[:, 0] - r[:, 2] / 2.0, r[:, 0] + r[:, 2] / 2.0
    xmin, xmax = r[:, 1] - r[:, 3] / 2.0, r[:, 1] + r[:, 3] / 2.0
    wm, hm = float(W - 1), float(H - 1)
    t00, t02 = (xmax - xmin) / wm, (xmin + xmax - wm) / wm
    t11, t12 = (ymax - ymin) / hm, (ymin + ymax - hm) / hm
    lin = -1.0 + 2.0 * np.arange(256, dtype=np.float64) / 255.0
    gx = lin[None, :] * t00[:, None] + t02[:, None]
    gy = lin[None, :] * t11[:, None] + t12[:, None]
    return ((gx + 1.0) * 0.5) * wm, ((gy + 1.0) * 0.5) * hm


def roi_sample64(img, yxhw_f32):
    """img [B,C,H,W] -> [B,C,256,256] float64."""
    img = np.asarray(img, np.float64)
    B, C, H, W = img.shape
    sx, sy = roi_points64(yxhw_f32, H, W)
    out = np.zeros((B, C, 256, 256), np.float64)
    for b in range(B):
        x0f, y0f = np.floor(sx[b]), np.floor(sy[b])
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        wx1, wy1 = sx[b] - x0f, sy[b] - y0f
        for dy, wy in ((0, 1.0 - wy1), (1, wy1)):
            yy = y0 + dy
            wyv = wy * ((yy >= 0) & (yy < H))
            yyc = np.clip(yy, 0, H - 1)
            for dx, wx in ((0, 1.0 - wx1), (1, wx1)):
                xx = x0 + dx
                wxv = wx * ((xx >= 0) & (xx < W))
                xxc = np.clip(xx, 0, W - 1)
                out[b] += img[b][:, yyc][:, :, xxc] * (wyv[:, None] * wxv[None, :])
    return out


def _lip(a):
    lx = np.abs(np.diff(a, axis=-1)).max() if a.shape[-1] > 1 else 0.0
    ly = np.abs(np.diff(a, axis=-2)).max() if a.shape[-2] > 1 else 0.0
    return float(lx), float(ly)


def lipschitz(img):
    """img [H,W] -> (Lx, Ly): the largest |I[y,x+1] - I[y,x]| and |I[y+1,x] - I[y,x]| of the image inside a one-pixel ring of
    zeros (what a zero-padding sampler interpolates over)."""
    return _lip(np.pad(np.asarray(img, np.float64), 1))


def lipschitz_interior(img):
    """The same without the ring: the slopes a sample point inside [0, W-1] x [0, H-1] can meet."""
    return _lip(np.asarray(img, np.float64))


def roi_bound(ref, Lx, Ly, H, W, s=1.0, bf16=False):
    """Bound on |got - ref| per output value of a float32 ROI sampler, ref = roi_sample64 (after (v - mean) / std for a colour).

    A sample point goes through about eight float32 roundings (the box corners, theta, linspace * theta + offset, + 1, * 0.5,
    * (size - 1)) on magnitudes up to the box extent, which all2yxhw's clamp limits to dim + 10 pixels: the point is off by at most
    dx = 8 * 2^-24 * (W + 10), dy = 8 * 2^-24 * (H + 10).  Bilinear interpolation with zero padding is continuous and piecewise
    bilinear, the padding band included, so the value moves by at most (Lx dx + Ly dy); the normalisation divides by s = std[c].
    The interpolation's and the normalisation's own roundings are covered by 4 * 2^-24 * max(|ref|, 1); a bf16 output adds its
    rounding, allowed as 2^-8 |ref| (bf16's unit roundoff: 8 significant bits)."""
    dx, dy = 8 * EPS32 * (W + 10), 8 * EPS32 * (H + 10)
    bound = (Lx * dx + Ly * dy) / s + 4 * EPS32 * np.maximum(np.abs(ref), 1.0)
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    return bound


def border_boxes(H, W):
    """The six boxes of test_roi_crop_with_boxes_over_every_frame_border."""
    return np.array([[H / 2, W / 2, H + 10, W + 10],              # over all four borders (x0 = -5 .. W + 4)
                     [20.0, 30.0, 60.0, 90.0],                     # top-left corner outside
                     [H - 10.0, W - 12.0, 50.0, 70.0],             # bottom-right corner outside
                     [H / 2, -2.0, 40.0, 9.0],                     # centred left of the frame
                     [H / 2, W + 1.5, 33.0, 11.0],                 # centred right of the frame
                     [H / 3, W / 3, 31.7, 47.3]], np.float32)      # inside


ROI_SIZES = ((480, 854), (37, 53), (2, 2))
ROI_KINDS = ("ramp_x", "ramp_y", "ramp_xy", "random")


def roi_image(kind, H, W, u8=False):
    """One test image set: (colour [3,H,W], P [H,W]) float32.  A ramp is all three colours and the P plane at once; ``u8``
    quantises the colours to bytes (returned as uint8 [3,H,W]; their value is float32(u8) / 255, P stays float32)."""
    x = np.arange(W, dtype=np.float64)[None, :] / (W - 1) + np.zeros((H, 1))
    y = np.arange(H, dtype=np.float64)[:, None] / (H - 1) + np.zeros((1, W))
    if kind == "random":
        rs = np.random.RandomState(H * W + 7)
        col, p = rs.rand(3, H, W), rs.rand(H, W)
    else:
        p = {"ramp_x": x, "ramp_y": y, "ramp_xy": (x + y) / 2.0}[kind]
        col = np.stack([p, p, p])
    p = p.astype(np.float32)
    if u8:
        return np.rint(col * 255.0).astype(np.uint8), p
    return col.astype(np.float32), p


def u8_unit(b):
    """The colour value of a byte: float32(b) / 255, correctly rounded."""
    return np.asarray(b, np.float32) / np.float32(255.0)


def roi_case(kind, H, W, u8=False):
    """Everything a check of one (image kind, frame size) needs, computed once: the six boxes, the inputs and, per channel c of
    the NHWC4 tile, the fp64 reference [6,256,256,4], the two Lipschitz pairs, s, and the mask of interior sample points."""
    boxes = border_boxes(H, W)
    B = len(boxes)
    col, p = roi_image(kind, H, W, u8)
    colf = u8_unit(col) if u8 else col
    img = np.concatenate([colf, p[None]], 0)                                    # [4,H,W] float32 values
    ref = roi_sample64(np.broadcast_to(img, (B,) + img.shape), boxes)           # [B,4,256,256]
    ref[:, :3] = (ref[:, :3] - MEAN[None, :, None, None]) / STD[None, :, None, None]
    sx, sy = roi_points64(boxes, H, W)
    inside = ((sy >= 1) & (sy <= H - 2))[:, :, None] & ((sx >= 1) & (sx <= W - 2))[:, None, :]     # [B,256,256]
    s = [STD[0], STD[1], STD[2], 1.0]
    return dict(boxes=boxes, col=col, p=p, img=img, ref=ref.transpose(0, 2, 3, 1), inside=inside, s=s,
                lip=[lipschitz(img[c]) for c in range(4)], lip_in=[lipschitz_interior(img[c]) for c in range(4)])


def roi_check(got, case, H, W, bf16=False):
    """got [6,256,256,4] -> (worst error / bound over every value, worst over the interior points; 0 if there are none)."""
    got = np.asarray(got, np.float64)
    worst_all, worst_in = 0.0, 0.0
    for c in range(4):
        ref = case["ref"][..., c]
        err = np.abs(got[..., c] - ref)
        worst_all = max(worst_all, float((err / roi_bound(ref, *case["lip"][c], H, W, case["s"][c], bf16)).max()))
        m = case["inside"]
        if m.any():
            worst_in = max(worst_in, float((err[m] / roi_bound(ref[m], *case["lip_in"][c], H, W, case["s"][c], bf16)).max()))
    return worst_all, worst_in


# ---------------------------------------------------------------- quality / state
QUALITY_N_OBJ = (1, 2, 7, 8, 9, 15, 16, 17, 31)
QUALITY_N_FRAMES = (1, 63, 64, 65, 130)
QUALITY_DECADES = (3, 7)


def quality_inputs(n_obj, n_frames, decades=3):
    """(scores [n_obj, n_frames] float32, counts [n_frames] float32): mixed signs, magnitudes log-uniform over 10^-d .. 10^d.

    d = 3 is the range the scores are specified with.  A float32 has 24 significant bits, 10^-3 .. 10^3 spans 20 binary orders
    and 31 terms add 5 more: every partial sum fits the 53 bits of a float64, so on that range EVERY summation order gives the
    same bits and a wrong order passes.  d = 7 (47 binary orders) makes the partial sums round, so the order shows: that is the
    set tests/test_oracle_front.py proves discriminating."""
    rs = np.random.RandomState(1000 * n_obj + n_frames + 7919 * decades)
    mag = 10.0 ** rs.uniform(-decades, decades, (n_obj, n_frames))
    sign = np.where(rs.rand(n_obj, n_frames) < 0.5, -1.0, 1.0)
    counts = (rs.randint(0, 9, n_frames) + rs.rand(n_frames) * (rs.rand(n_frames) < 0.3)).astype(np.float32)
    return (mag * sign).astype(np.float32), counts


def quality_ref(scores_f32):
    """scores [n_obj, n_frames] float32 -> float64 [n_frames]: the reference fills a float64 [n_frames, n_obj] array with the
    float32 scores and takes .mean(1) (utils/utils_agent.py:116-120)."""
    return np.asarray(np.asarray(scores_f32, np.float32).T, np.float64).copy().mean(1)


def quality_sequential(scores_f32):
    """The same mean from a plain left-to-right float64 sum: what a kernel without numpy's pairwise order computes."""
    s = np.asarray(scores_f32, np.float32).astype(np.float64)
    acc = s[0].copy()
    for o in range(1, s.shape[0]):
        acc = acc + s[o]
    return acc / float(s.shape[0])


# ---------------------------------------------------------------- head
def head_ref(res5_nhwc, fc_w, fc_b):
    """res5 [B,8,8,2048], fc_w [1,2048] (or [2048]), fc_b [1] -> (pooled [B,2048], scores [B]) float64."""
    x = np.asarray(res5_nhwc, np.float64)
    pooled = x.reshape(x.shape[0], 64, x.shape[3]).mean(1)
    w = np.asarray(fc_w, np.float64).reshape(-1)
    return pooled, pooled @ w + float(np.asarray(fc_b, np.float64).reshape(-1)[0])
