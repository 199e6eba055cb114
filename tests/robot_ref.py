"""numpy restatement of the scribble robot's rules (include/ivosw.h, "scribble robot"; csrc/robot.hip; utils/robot.py), written from their
statement, not from the kernel:

  error_plane     gt == o and pred != o (pred None: all background).
  thin            Zhang-Suen (1984) pixel by pixel: the rule is ``deletable`` on one pixel's eight neighbours, sub-iteration 1 then 2 on the
                  plane as it was before the sub-iteration, everything outside the image 0, until an iteration deletes nothing, at most
                  max(H, W) iterations; (skeleton, iters) with iters = the number of iterations that deleted a pixel, -1 at the cap.
  thin_fast       the same rule applied to all pixels at once: ``deletable`` tabulated over the 256 neighbourhoods, the neighbourhood code
                  of every pixel from eight shifted views (tools/robot_probe.py times it as the host side).
  pack_bits / points_of   the kernel's output forms: the uint32 bit plane and the (y << 16) | x list in raster order.
  longest_paths / paths_from_points   the component, double-BFS and resampling step of utils/robot.py, restated with plain lists.

davisinteractive and skimage are not installed where this is built: none of this is compared with the library's own robot."""
import numpy as np

# P2 .. P9 = N, NE, E, SE, S, SW, W, NW as (dy, dx)
NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


EIGHT = np.ones((3, 3), bool)                 # scipy.ndimage.label's structure for 8-connectivity


def blob(H, W, seed):
    """Random blobs with numpy alone: uniform noise on (H + 4) x (W + 4), the mean of every 5 x 5 window, thresholded at 0.5 (the blobs
    touch the borders)."""
    n = np.random.default_rng(seed).random((H + 4, W + 4))
    c = np.cumsum(np.cumsum(np.pad(n, ((1, 0), (1, 0))), 0), 1)
    box = c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]
    return box / 25.0 > 0.5


def error_plane(gt, pred, obj):
    """bool [H,W] from uint8 label maps [H,W]."""
    return (gt == obj) if pred is None else ((gt == obj) & (pred != obj))


def deletable(p, sub):
    """The rule on one set pixel: ``p`` = (P2, .., P9) as 0 / 1, ``sub`` = 0 for sub-iteration 1, 1 for sub-iteration 2."""
    p2, p3, p4, p5, p6, p7, p8, p9 = p
    b = sum(p)
    a = sum(1 for k in range(8) if p[k] == 0 and p[(k + 1) % 8] == 1)
    if not (2 <= b <= 6 and a == 1):
        return False
    if sub == 0:
        return p2 * p4 * p6 == 0 and p4 * p6 * p8 == 0
    return p2 * p4 * p8 == 0 and p2 * p6 * p8 == 0


def thin(plane):
    """(skeleton bool [H,W], iters) pixel by pixel."""
    H, W = plane.shape
    img = [[0] * (W + 2) for _ in range(H + 2)]                   # a zero border: outside the image is 0
    alive = []
    for y, x in zip(*np.nonzero(plane)):
        img[y + 1][x + 1] = 1
        alive.append((int(y) + 1, int(x) + 1))
    iters = -1
    for it in range(max(H, W)):
        deleted = False
        for sub in (0, 1):
            gone = [(y, x) for y, x in alive if deletable([img[y + dy][x + dx] for dy, dx in NEIGHBOURS], sub)]
            if gone:                                              # decided on the old plane, applied afterwards
                deleted = True
                for y, x in gone:
                    img[y][x] = 0
                alive = [q for q in alive if img[q[0]][q[1]]]
        if not deleted:
            iters = it
            break
    out = np.zeros((H, W), bool)
    for y, x in alive:
        out[y - 1, x - 1] = True
    return out, iters


_TABLE = None


def _table():
    """bool [2,256]: ``deletable`` for every neighbourhood code sum(P_(k+2) << k)."""
    global _TABLE
    if _TABLE is None:
        _TABLE = np.array([[deletable([(code >> k) & 1 for k in range(8)], sub) for code in range(256)] for sub in (0, 1)])
    return _TABLE


def thin_fast(plane):
    """``thin`` with every pixel of a sub-iteration decided in one numpy expression."""
    H, W = plane.shape
    tab = _table()
    pad = np.zeros((H + 2, W + 2), np.uint8)
    pad[1:-1, 1:-1] = plane
    iters = -1
    for it in range(max(H, W)):
        deleted = False
        for sub in (0, 1):
            code = np.zeros((H, W), np.uint8)
            for k, (dy, dx) in enumerate(NEIGHBOURS):
                code |= pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] << k
            gone = tab[sub][code] & (pad[1:-1, 1:-1] == 1)
            if gone.any():
                deleted = True
                pad[1:-1, 1:-1][gone] = 0
        if not deleted:
            iters = it
            break
    return pad[1:-1, 1:-1].astype(bool), iters


def pack_bits(plane):
    """uint32 [H, ceil(W/32)]: bit (x & 31) of word (x >> 5) of row y."""
    H, W = plane.shape
    WW = (W + 31) // 32
    wide = np.zeros((H, WW * 32), np.uint64)
    wide[:, :W] = plane
    return (wide.reshape(H, WW, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def unpack_bits(words, W):
    H, WW = words.shape
    return (((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(H, WW * 32)[:, :W]).astype(bool)


def points_of(plane):
    """int32 [count]: (y << 16) | x in ascending raster order."""
    ys, xs = np.nonzero(plane)
    return ((ys.astype(np.int64) << 16) | xs).astype(np.int32)


def skeleton(gt, pred, obj):
    """One unit the slow way: (bit plane uint32 [H,WW], points int32 [count], iters)."""
    sk, iters = thin(error_plane(gt, pred, obj))
    return pack_bits(sk), points_of(sk), iters


# ------------------------------------------------------------------------------------------------ the path step
def components(pixels):
    """8-connected components of a raster-ordered pixel list [(y, x), ...]: lists of pixels, each in raster order, the components in the
    order of their first pixels."""
    index = {p: i for i, p in enumerate(pixels)}
    label = [-1] * len(pixels)
    comps = []
    for i, p in enumerate(pixels):
        if label[i] >= 0:
            continue
        label[i] = len(comps)
        stack, members = [p], []
        while stack:
            y, x = stack.pop()
            members.append((y, x))
            for dy, dx in NEIGHBOURS:
                j = index.get((y + dy, x + dx))
                if j is not None and label[j] < 0:
                    label[j] = len(comps)
                    stack.append((y + dy, x + dx))
        comps.append(sorted(members))
    return comps


def bfs(members, start):
    """(distance, parent) dicts over the component from ``start``, neighbours visited in the order N, NE, E, SE, S, SW, W, NW."""
    inside = set(members)
    dist, parent, queue = {start: 0}, {start: None}, [start]
    for y, x in queue:                                            # the list grows while it is walked: a FIFO
        for dy, dx in NEIGHBOURS:
            q = (y + dy, x + dx)
            if q in inside and q not in dist:
                dist[q], parent[q] = dist[(y, x)] + 1, (y, x)
                queue.append(q)
    return dist, parent


def farthest(dist):
    """The farthest node; ties go to the lower raster index."""
    best = max(dist.values())
    return min(p for p, d in dist.items() if d == best)


def longest_path(members):
    """A longest shortest path of one component by double BFS from its first pixel: the node list from the first BFS's farthest node to
    the second's."""
    a = farthest(bfs(members, members[0])[0])
    dist, parent = bfs(members, a)
    node, path = farthest(dist), []
    while node is not None:
        path.append(node)
        node = parent[node]
    return path[::-1]


def longest_paths(pixels, min_nb_nodes=4, max_paths=2):
    """The node lists (before resampling) that survive: components of at least ``min_nb_nodes`` pixels, the ``max_paths`` longest paths,
    longest first, ties to the component with the lower first pixel."""
    paths = [longest_path(c) for c in components(pixels) if len(c) >= min_nb_nodes]
    order = sorted(range(len(paths)), key=lambda k: (-len(paths[k]), k))          # (components come in the order of their first pixels)
    return [paths[k] for k in order[:max_paths]]


def resample(path, nb_points):
    idx = np.unique(np.linspace(0, len(path) - 1, min(int(nb_points), len(path))).round().astype(int))
    return [path[i] for i in idx]


def paths_from_points(points, count, size, object_id, min_nb_nodes=4, max_paths=2, nb_points=8):
    H, W = size
    pts = np.asarray(points[:count]).astype(np.int64) & 0xffffffff
    pixels = [(int(v >> 16), int(v & 0xffff)) for v in pts]
    out = []
    for path in longest_paths(pixels, min_nb_nodes, max_paths):
        nodes = path if nb_points is None else resample(path, nb_points)
        out.append(dict(path=[[(x + 0.5) / W, (y + 0.5) / H] for y, x in nodes], object_id=int(object_id), start_time=0, end_time=0))
    return out
