"""TEST INFRASTRUCTURE (never imported by the product path): deterministic (gt, pred) label-map pairs that put object
pixels where the J/F kernels of csrc/metrics.hip take another path, and the probes that show they do.

Every builder returns a ``Case``: uint8 ``gt`` / ``pred`` [N,H,W], ``nb_objects`` (None = ids from the labels) and the
boundary tolerance ``bound_th`` in pixels.  Nearly every builder ends with ``_both_ways``: each frame appears a second
time with the two maps swapped, so whatever one map shows the other shows too.  The comparison reference is
oracle/jf_oracle.py (``counts`` below collects its six integer intermediates per frame and object); what pins THAT at
the frame's edges is the per-pixel restatement ``brute_counts`` (tests/test_oracle_jf_cases.py).

Where the kernels branch (csrc/metrics.hip):
  * a lane owns 16 pixels of a row, a wave 4 rows of a 1024-pixel segment, a block 16 rows; the east neighbour of a
    segment's last pixel (columns 1023 | 1024, 2047 | 2048) is a separate byte load, everywhere else a lane shuffle
  * last column: b = seg ^ south; last row: b = seg ^ east; the corner is 0
  * a 16-byte load that would pass the end of the buffer is assembled byte by byte (the last rows of the last frame)
  * the byte compare is SWAR arithmetic on four labels per word (carries: ids and labels >= 128)
  * the counts of a wave travel as two 16-bit halves of one word (at most 4096 each)
  * matching ORs (2r+1) row smears of the other map's bitmap words, clipped at the frame and at the row's first / last word
"""
import collections
import functools

import numpy as np

from oracle import jf_oracle as jo

Case = collections.namedtuple("Case", "gt pred nb_objects bound_th")


# ------------------------------------------------------------------------------------------------ reference counts
def counts(gt, pred, ids, r):
    """int64 [N, len(ids), 6] from the oracle's own functions: |gt & pred|, |gt | pred|, #pred boundary, #gt boundary, pred
    boundary inside dil(gt boundary), gt boundary inside dil(pred boundary)."""
    N = gt.shape[0]
    se = jo.disk(r)
    out = np.zeros((N, len(ids), 6), np.int64)
    for n in range(N):
        for o, oid in enumerate(ids):
            g, p = gt[n] == oid, pred[n] == oid
            if not (g.any() or p.any()):
                continue
            bg, bp = jo.seg2bmap(g), jo.seg2bmap(p)
            m_fg = (bp & jo.binary_dilation(bg, se)).sum() if bg.any() and bp.any() else 0
            m_gt = (bg & jo.binary_dilation(bp, se)).sum() if bg.any() and bp.any() else 0
            out[n, o] = [(g & p).sum(), (g | p).sum(), bp.sum(), bg.sum(), m_fg, m_gt]
    return out


def j_and_f(c):
    """J and F [N, O] from the six counts, by the oracle's own expressions (jo.batched_jaccard's ratio, jo.pr_to_f): what
    jo.batched_jaccard / jo.batched_f_measure return with average_over_objects=False, without running the dilations again."""
    j = np.empty(c.shape[:2], np.float64)
    f = np.empty(c.shape[:2], np.float64)
    for idx in np.ndindex(j.shape):
        inter, union, n_fg, n_gt, m_fg, m_gt = (c[idx][k] for k in range(6))
        j[idx] = 1.0 if np.isclose(union, 0) else inter / union
        f[idx] = jo.pr_to_f(n_fg, n_gt, m_fg, m_gt)
    return j, f


def brute_counts(g, p, r):
    """The six counts of one boolean pair from the definition alone, pixel by pixel and pair by pair (small frames only)."""
    H, W = g.shape

    def bmap(s):
        b = np.zeros((H, W), bool)
        for y in range(H):
            for x in range(W):
                if y == H - 1 and x == W - 1:
                    continue
                if y == H - 1:
                    b[y, x] = s[y, x] != s[y, x + 1]
                elif x == W - 1:
                    b[y, x] = s[y, x] != s[y + 1, x]
                else:
                    b[y, x] = s[y, x] != s[y, x + 1] or s[y, x] != s[y + 1, x] or s[y, x] != s[y + 1, x + 1]
        return b

    bg, bp = bmap(g), bmap(p)
    pg, pp = np.argwhere(bg), np.argwhere(bp)

    def matched(src, dst):
        return sum(1 for (y, x) in src if any((y - v) ** 2 + (x - u) ** 2 <= r * r for (v, u) in dst))

    return [int((g & p).sum()), int((g | p).sum()), len(pp), len(pg), matched(pp, pg), matched(pg, pp)]


# ------------------------------------------------------------------------------------------------ probes
def object_mask(a, ids=None):
    a = np.asarray(a)
    return ((a > 0) & (a < 255)) if ids is None else np.isin(a, np.asarray(ids))


def border_pixels(a, ids=None):
    """Object pixels on the frame's border: dict top / bottom / left / right / corner (the bottom-right pixel)."""
    m = object_mask(a, ids)
    return dict(top=int(m[:, 0, :].sum()), bottom=int(m[:, -1, :].sum()), left=int(m[:, :, 0].sum()),
                right=int(m[:, :, -1].sum()), corner=int(m[:, -1, -1].sum()))


def column_pixels(a, col, ids=None):
    m = object_mask(a, ids)
    return int(m[:, :, col].sum()) if col < a.shape[2] else 0


def max_per_wave(gt, pred, ids):
    """Largest intersection / union count that one wave of the boundary kernel (4 rows x 1024 columns, one object) adds up."""
    N, H, W = gt.shape
    best = [0, 0]
    for oid in ids:
        g, p = gt == oid, pred == oid
        for k, m in enumerate((g & p, g | p)):
            for y0 in range(0, H, 4):
                for x0 in range(0, W, 1024):
                    best[k] = max(best[k], int(m[:, y0:y0 + 4, x0:x0 + 1024].sum(axis=(1, 2)).max()))
    return tuple(best)


def empty_word_share(gt, pred, ids):
    """Share of the 32-pixel boundary bitmap words (both maps, every object) that hold no boundary pixel."""
    tot = empty = 0
    for a in (gt, pred):
        for n in range(a.shape[0]):
            for oid in ids:
                b = jo.seg2bmap(a[n] == oid)
                W = b.shape[1]
                bw = np.zeros((b.shape[0], (W + 31) // 32 * 32), bool)
                bw[:, :W] = b
                words = bw.reshape(b.shape[0], -1, 32).any(axis=2)
                tot += words.size
                empty += int((~words).sum())
    return empty / tot


def slow_path_loads(N, H, W):
    """How many 16-byte lane loads of the last frame would pass the end of the buffer (byte-by-byte path of load16)."""
    total = N * H * W
    n = 0
    for y in range(H):
        for x0 in range(0, W, 16):
            n += ((N - 1) * H + y) * W + x0 + 16 > total
    return n


def _both_ways(gt, pred):
    return np.concatenate([gt, pred]).astype(np.uint8), np.concatenate([pred, gt]).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ borders
BORDER_H = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)        # 4 rows per wave, 16 per block
BORDER_W = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)     # 16 pixels per lane, 32 per bitmap word
# three diagonals of the H x W table: every H and every W three times, 1 x 1, 1 x W and H x 1 among them
BORDER_SHAPES = [(BORDER_H[i], BORDER_W[(i + k) % 11], r) for k, r in ((0, 1), (3, 2), (7, 3)) for i in range(11)]


@functools.lru_cache(maxsize=None)
def border_case(H, W, r):
    """Object 1 on the frame's borders.  Frames (gt | pred), then all of them again with the maps swapped:
    full | full, full | empty, a rectangle in each corner | a smaller one in the same corner, a band along each edge | a thicker one,
    the last row | the last row without its first pixel, the last column | without its first pixel, the pixel (H-1, W-1) | that pixel
    and the one above, the last-row and last-column stripes | empty (an object of one map only)."""
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    fr = []

    def add(fg, fp):
        g, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        fg(g)
        fp(p)
        fr.append((g, p))

    def setter(ys, xs):
        def f(a):
            a[ys, xs] = 1
        return f

    def nothing(a):
        pass

    full = setter(slice(None), slice(None))
    add(full, full)
    add(full, nothing)
    for top in (True, False):
        for left in (True, False):
            def rect(h, w):
                return setter(slice(0, h) if top else slice(H - h, H), slice(0, w) if left else slice(W - w, W))
            add(rect(h2, w2), rect(max(1, h2 - 1), max(1, w2 - 1)))
    q = W // 4
    add(setter(slice(0, h2), slice(q, W - q)), setter(slice(0, min(H, h2 + 1)), slice(q, W - q)))                 # top edge
    add(setter(slice(H - h2, H), slice(q, W - q)), setter(slice(max(0, H - h2 - 1), H), slice(q, W - q)))         # bottom edge
    q = H // 4
    add(setter(slice(q, H - q), slice(0, w2)), setter(slice(q, H - q), slice(0, min(W, w2 + 1))))                 # left edge
    add(setter(slice(q, H - q), slice(W - w2, W)), setter(slice(q, H - q), slice(max(0, W - w2 - 1), W)))         # right edge
    add(setter(H - 1, slice(None)), setter(H - 1, slice(1, None)))
    add(setter(slice(None), W - 1), setter(slice(1, None), W - 1))
    add(setter(H - 1, W - 1), setter(slice(max(0, H - 2), H), W - 1))
    add(setter(H - 1, slice(None)), nothing)
    add(setter(slice(None), W - 1), nothing)
    gt, pred = _both_ways(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]))
    return Case(gt, pred, 1, r)


# ------------------------------------------------------------------------------------------------ the 1024-pixel seam
SEAM_SHAPES = [(H, W) for W in (1025, 1040, 1100, 2049) for H in (5, 17)]


def seam_columns(W):
    """Edge columns: around the seam, and 1007 .. 1009 - the border between lanes 62 and 63, whose neighbour bit crosses a select."""
    return list((1007, 1008, 1009, 1022, 1023, 1024, 1025, 1026) + ((2046, 2047, 2048, 2049) if W == 2049 else ()))


@functools.lru_cache(maxsize=None)
def seam_case(H, W):
    """Object 1 around the columns where a wave's 1024-pixel segment ends.  With cols = 1007..1009, 1022..1026 (and 2046..2049 at W = 2049):
    a vertical edge at every column c (the object is [0, c) in gt) against an edge at another column of the list in pred, once over
    the whole height and once over the inner rows, and the same with the object on the right ([c, W)); a diagonal edge through each
    seam (x < seam - H // 2 + y against x < seam + H // 2 - y); one-pixel columns at 1023 | 1024 and 1024 | 1023 (2047 | 2048 too).
    Then every frame again with the maps swapped: each edge column occurs in gt and in pred."""
    cols = seam_columns(W)
    fr = []
    yy, xx = np.mgrid[0:H, 0:W]
    for i, c in enumerate(cols):
        cp = cols[(i + 2) % len(cols)]
        for right in (False, True):
            for inner in (False, True):
                g, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
                rows = slice(1, H - 1) if inner else slice(None)
                g[rows, c:] = 1
                p[rows, cp:] = 1
                if not right:
                    g[rows], p[rows] = 1 - g[rows], 1 - p[rows]
                fr.append((g, p))
    seams = (1024, 2048) if W == 2049 else (1024,)
    for s in seams:
        fr.append(((xx < s - H // 2 + yy).astype(np.uint8), (xx < s + H // 2 - yy).astype(np.uint8)))
        fr.append(((xx >= s - H // 2 + yy).astype(np.uint8), (xx >= s + H // 2 - yy + 1).astype(np.uint8)))
        for a, b in ((s - 1, s), (s, s - 1)):
            g, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
            g[:, a] = 1
            p[:, b] = 1
            fr.append((g, p))
            g, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
            g[1:H - 1, a] = 1
            p[2:, b] = 1
            fr.append((g, p))
    gt, pred = _both_ways(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]))
    return Case(gt, pred, 1, 2)


# ------------------------------------------------------------------------------------------------ end of the buffer
TAIL_SHAPES = [(1, 1, 5), (1, 3, 5), (1, 5, 15), (1, 3, 17), (1, 5, 33), (1, 3, 1), (1, 1, 1), (1, 5, 1025),
               (2, 1, 5), (2, 3, 5), (2, 5, 15), (2, 3, 17), (2, 5, 31), (2, 3, 2), (3, 1, 1), (2, 5, 1025), (2, 3, 1100)]


@functools.lru_cache(maxsize=None)
def tail_case(N, H, W):
    """W < 16 or W % 16 != 0, H odd.  Object 1 fills the first min(W, 16) pixels of every odd row and of row 0 of every frame but
    the first; even rows hold it nowhere near their end.  The 16 bytes a lane loads at the end of an even row therefore run into
    object pixels of row y + 1 (of frame n + 1 after the last row): without the valid-pixel mask they would be counted.  The last
    rows of the last frame cannot load 16 bytes at all (slow path of load16).  pred: the same stripes without their first pixel,
    and its even rows start with a pixel of their own.  No swap: the stripes must stay in the rows after the empty ones."""
    assert H % 2 == 1 and (W < 16 or W % 16)
    k = min(W, 16)
    gt, pred = np.zeros((N, H, W), np.uint8), np.zeros((N, H, W), np.uint8)
    gt[:, 1::2, :k] = 1
    gt[1:, 0, :k] = 1
    pred[:, 1::2, 1:k] = 1
    pred[1:, 0, 1:k] = 1
    pred[:, 0::2, 0] = 1
    return Case(gt, pred, 1, 1)


# ------------------------------------------------------------------------------------------------ ids and object count
UNIQUE_IDS = (1, 7, 127, 128, 200, 254)
CABI_IDS = (200, 7, 0, 255, 128, 127, 1, 254, 129, 64, 191, 2)          # not ascending; 0 and 255 are ordinary bytes at this level


@functools.lru_cache(maxsize=None)
def iid_bytes_case():
    """Every pixel of both maps drawn iid from all 256 byte values (W = 70: a ragged last lane and last word)."""
    rs = np.random.RandomState(256)
    return Case(rs.randint(0, 256, (2, 19, 70)).astype(np.uint8), rs.randint(0, 256, (2, 19, 70)).astype(np.uint8), 32, 1)


def _blocks(rs, N, H, W, values, n_rect):
    a = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for _ in range(n_rect):
            y, x = rs.randint(0, H), rs.randint(0, W)
            a[n, y:y + rs.randint(1, H // 2 + 1), x:x + rs.randint(1, W // 3 + 1)] = values[rs.randint(len(values))]
    return a


@functools.lru_cache(maxsize=None)
def unique_ids_case():
    """Blocks of the ids {1, 7, 127, 128, 200, 254}, background and a 255 void block; nb_objects = None (ids from np.unique)."""
    rs = np.random.RandomState(254)
    vals = UNIQUE_IDS + (0, 255)
    gt = _blocks(rs, 2, 20, 45, vals, 14)
    pred = np.where(rs.rand(2, 20, 45) < 0.8, gt, _blocks(rs, 2, 20, 45, vals, 14)).astype(np.uint8)
    for v in UNIQUE_IDS:                       # every id certainly present in gt
        gt[0, 19, 2 * UNIQUE_IDS.index(v)] = v
    gt[1, :3, :6] = 255
    return Case(gt, pred, None, 2)


@functools.lru_cache(maxsize=None)
def many_objects_case():
    """32 objects (the kernel's maximum): a 4 x 8 grid of blocks with ids 1..32, shifted by one pixel in pred, plus iid noise."""
    rs = np.random.RandomState(32)
    H, W = 18, 70
    yy, xx = np.mgrid[0:H, 0:W]
    gt = (1 + np.minimum(yy // 5, 3) * 8 + np.minimum(xx // 9, 7)).astype(np.uint8)
    gt = np.stack([gt, gt[::-1].copy()])
    pred = np.roll(gt, (1, 1), axis=(1, 2))
    noise = rs.rand(*gt.shape) < 0.05
    pred = np.where(noise, rs.randint(0, 34, gt.shape), pred).astype(np.uint8)
    return Case(gt, pred, 32, 1)


# ------------------------------------------------------------------------------------------------ dense maps
@functools.lru_cache(maxsize=None)
def checkerboard_case(H=21, W=70):
    """One-pixel checkerboard against itself, its complement and its shift by a row; every bitmap word is non-empty."""
    yy, xx = np.mgrid[0:H, 0:W]
    cb = ((yy + xx) % 2).astype(np.uint8)
    gt = np.stack([cb, cb, cb])
    pred = np.stack([cb, 1 - cb, np.roll(cb, 1, axis=0)])
    gt[2, 0] = 0
    return Case(*_both_ways(gt, pred), 1, 1)


@functools.lru_cache(maxsize=None)
def coin_flip_case(H=21, W=1100):
    """iid labels in {0, 1, 2} (p = 0.5 for object 1), across the segment seam."""
    rs = np.random.RandomState(50)
    gt = rs.choice(np.array([0, 1, 2], np.uint8), (2, H, W), p=[0.25, 0.5, 0.25])
    pred = rs.choice(np.array([0, 1, 2], np.uint8), (2, H, W), p=[0.25, 0.5, 0.25])
    return Case(gt, pred, 2, 1)


@functools.lru_cache(maxsize=None)
def full_wave_case():
    """16 x 1024 and 32 x 2048, object 1 everywhere in both maps: every wave adds up 4 x 1024 = 4096 intersection and 4096 union
    pixels, the most the 16-bit halves of its packed counter ever hold.  A second frame without one pixel in each map."""
    out = []
    for H, W in ((16, 1024), (32, 2048)):
        gt, pred = np.ones((2, H, W), np.uint8), np.ones((2, H, W), np.uint8)
        gt[1, H - 1, W - 1] = 0
        pred[1, 0, 0] = 0
        out.append(Case(gt, pred, 1, 1))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ radius
RADII = (0, 1, 7, 8, 9, 31, 32)
RADIUS_W = 130                              # five bitmap words, the last with two pixels
RADIUS_PARTS = ("row", "col", "rim", "frame")


def half_widths(r):
    """Half width of disk(r) at row offset |dy|: the largest w with w^2 + dy^2 <= r^2."""
    return [int(np.floor(np.sqrt(r * r - d * d) + 1e-9)) for d in range(r + 1)]


def rim_offsets(r, part):
    hw = half_widths(r)
    if part == "row":
        return [(0, r + k) for k in range(3)]
    if part == "col":
        return [(r + k, 0) for k in range(3)]
    return [(dy, hw[dy] + k) for dy in sorted({d for d in (1, r // 2, r - 1) if 0 < d <= r}) for k in range(2)]


@functools.lru_cache(maxsize=None)
def radius_case(r, part):
    """Tolerance r at W = 130 (the scipy dilation by disk(32) costs ~ 0.1 us per pixel and footprint element: the frames are as low
    as the part allows, and a case holds a few of them).  An isolated object pixel at (y, x) has the boundary {y-1, y} x {x-1, x};
    two of them, one per map, at offset (dy, dx) have boundary pixels at every offset (dy + {-1, 0, 1}, dx + {-1, 0, 1}), so the
    matched counts change exactly where the disk ends.  Both roles are in every frame: seen from pred's boundary the other map lies
    at (-dy, -dx), seen from gt's at (+dy, +dx).
      row    dy = 0, dx = r, r + 1, r + 2 from x = 30: the pair straddles word borders (H = 6)
      col    dx = 0, dy = r, r + 1, r + 2 (H = r + 8)
      rim    the disk's corners: dy in {1, r // 2, r - 1}, dx = hw[dy], hw[dy] + 1 (H = r + 8)
      frame  2 x 2 objects in every corner and at the middle of every edge of gt, in pred moved inwards by r // 2 + 1: boundary pixels
             within r of every border, the smear clipped at yy < 0, yy >= H, the first and the last word; and the same swapped (H = 40)"""
    W = RADIUS_W
    if part != "frame":
        offs = rim_offsets(r, part)
        H = 6 if part == "row" else r + 8
        gt, pred = np.zeros((len(offs), H, W), np.uint8), np.zeros((len(offs), H, W), np.uint8)
        for n, (dy, dx) in enumerate(offs):
            gt[n, 3, 30] = 1
            pred[n, 3 + dy, 30 + dx] = 1
        return Case(gt, pred, 1, r)
    H = 40
    g, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    s = r // 2 + 1
    for y in (0, H // 2 - 1, H - 2):
        for x in (0, W // 2 - 1, W - 2):
            if (y, x) == (H // 2 - 1, W // 2 - 1):
                continue
            g[y:y + 2, x:x + 2] = 1
            py = y + (s if y == 0 else -s if y == H - 2 else 0)
            px = x + (s if x == 0 else -s if x == W - 2 else 0)
            p[py:py + 2, px:px + 2] = 1
    return Case(*_both_ways(g[None], p[None]), 1, r)


# ------------------------------------------------------------------------------------------------ workspace reuse
@functools.lru_cache(maxsize=None)
def reuse_cases():
    """(large dense, small sparse): three objects iid over 4 x 64 x 300 (every bitmap word of the workspace set), then one 2 x 2
    object at 1 x 7 x 40 - its bitmaps lie where the first call's words were."""
    rs = np.random.RandomState(7)
    big = Case(rs.randint(0, 4, (4, 64, 300)).astype(np.uint8), rs.randint(0, 4, (4, 64, 300)).astype(np.uint8), 3, 8)
    g, p = np.zeros((1, 7, 40), np.uint8), np.zeros((1, 7, 40), np.uint8)
    g[0, 2:4, 20:22] = 2
    p[0, 3:5, 21:23] = 2
    return big, Case(g, p, 3, 8)
