"""numpy restatement of ``ivosw_robot_paths``' rule (include/ivosw.h, "robot paths"), written from its statement, not from the kernel: the
path step of tests/robot_ref.py with the FIFO BFS stated level by level, so that nothing depends on an order of execution.

  neighbour_table   int [n,8]: the node index of every node's neighbour in the directions N, NE, E, SE, S, SW, W, NW, -1 where there is
                    none, from the raster-ordered unsigned keys (y << 16) | x.
  labels            the lowest node index of every node's 8-connected component (minimum propagation until nothing changes).
  sweep             the level-synchronous, multi-source BFS: ``parent[q]`` is the neighbour at distance ``dist[q] - 1`` that stands first
                    in the queue; the nodes of level d + 1 stand in ascending order of (queue position of parent, direction parent -> q).
                    One sweep serves all components at once: the relative order inside a component depends on that component alone.
  longest_paths     components, min_nb_nodes, double sweep, selection: the node lists robot_ref.longest_paths gives.
  resample_indices  rint(fl64(i * fl64((len - 1) / (n - 1)))) for i < n - 1, len - 1 for the last (n == 1: 0), equal neighbours dropped.
  device_paths      the kernel's three outputs (nodes, lens, status) for a batch of units, padding and (-1, -1) fills included."""
import numpy as np

NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def keys_of(points, count):
    """The unsigned keys of a unit: int64 [count] from the int32 words (y << 16) | x."""
    return np.asarray(points[:count]).astype(np.int64) & 0xffffffff


def neighbour_table(keys):
    keys = np.asarray(keys, np.int64)
    n = len(keys)
    y, x = keys >> 16, keys & 0xffff
    nbr = np.full((n, 8), -1, np.int64)
    for d, (dy, dx) in enumerate(NEIGHBOURS):
        yy, xx = y + dy, x + dx
        ok = (yy >= 0) & (yy <= 0xffff) & (xx >= 0) & (xx <= 0xffff)
        want = (yy << 16) | xx
        pos = np.searchsorted(keys, want)
        hit = ok & (pos < n)
        hit[hit] = keys[pos[hit]] == want[hit]
        nbr[hit, d] = pos[hit]
    return nbr


def labels(nbr):
    n = len(nbr)
    lab = np.arange(n)
    while True:
        cand = np.where(nbr >= 0, lab[np.maximum(nbr, 0)], n).min(1, initial=n)
        new = np.minimum(lab, cand)
        new = new[new]                                            # (a shortcut only: the fixed point is the same)
        if (new == lab).all():
            return lab
        lab = new


def sweep(nbr, lab, sources):
    """(mk, queue, far): ``mk[q]`` = ((queue position of parent + 1) << 3) | direction (0 for a source, -1 for a node not reached),
    ``queue`` the nodes in queue order, ``far[root]`` = (level, node) of the farthest node of the component with that root, ties to the
    lower node."""
    n = len(nbr)
    big = np.iinfo(np.int64).max
    mk = np.full(n, big)
    queue = [int(s) for s in sources]
    mk[queue] = 0
    far = {int(lab[s]): (0, int(s)) for s in queue}
    p0, p1, level = 0, len(queue), 0
    while p1 > p0:
        level += 1
        q = nbr[queue[p0:p1]]                                     # [F,8]
        key = ((np.arange(p0, p1)[:, None] + 1) << 3) | np.arange(8)[None]
        valid = q >= 0
        np.minimum.at(mk, q[valid], key[valid])
        win = valid & (mk[np.maximum(q, 0)] == key)
        new = q[win]                                              # row-major: ascending key
        for node in new.tolist():
            root = int(lab[node])
            if far[root][0] < level or node < far[root][1]:
                far[root] = (level, node)
        queue.extend(new.tolist())
        p0, p1 = p1, len(queue)
    mk[mk == big] = -1
    return mk, queue, far


def _paths(keys, min_nb_nodes, max_paths):
    """The selected paths of one unit as lists of node indices, a -> b, longest first."""
    keys = np.asarray(keys, np.int64)
    if len(keys) == 0:
        return []
    nbr = neighbour_table(keys)
    lab = labels(nbr)
    size = np.bincount(lab, minlength=len(keys))
    roots = [r for r in range(len(keys)) if lab[r] == r and size[r] >= int(min_nb_nodes)]
    if not roots:
        return []
    _, _, far1 = sweep(nbr, lab, roots)
    mk, queue, far2 = sweep(nbr, lab, [far1[r][1] for r in roots])
    order = sorted(roots, key=lambda r: (-(far2[r][0] + 1), r))[:int(max_paths)]
    out = []
    for r in order:
        node, path = far2[r][1], []
        while True:
            path.append(node)
            if mk[node] == 0:
                break
            node = queue[(int(mk[node]) >> 3) - 1]
        out.append(path[::-1])
    return out


def longest_paths(pixels, min_nb_nodes=4, max_paths=2):
    """robot_ref.longest_paths by the level-synchronous statement: ``pixels`` = [(y, x), ...] in raster order -> lists of (y, x)."""
    keys = np.array([(y << 16) | x for y, x in pixels], np.int64)
    return [[(int(keys[i] >> 16), int(keys[i] & 0xffff)) for i in path] for path in _paths(keys, min_nb_nodes, max_paths)]


def resample_indices(length, nb_points):
    n = min(int(nb_points), int(length))
    if n == 1:
        return [0]
    step = np.float64(length - 1) / np.float64(n - 1)
    idx = [int(np.rint(np.float64(i) * step)) for i in range(n - 1)] + [length - 1]
    return [v for i, v in enumerate(idx) if i == 0 or v != idx[i - 1]]


def device_paths(points, counts, min_nb_nodes, max_paths, nb_points, slot):
    """``ivosw_robot_paths``' outputs for host ``points`` int32 [m,cap] and ``counts`` int32 [m]: (nodes int32 [m,max_paths,slot,2] =
    (x, y), lens int32 [m,max_paths], status int32 [m]).  ``nb_points`` None or <= 0: every node."""
    points, counts = np.asarray(points), np.asarray(counts)
    m, cap = points.shape
    nodes = np.full((m, max_paths, slot, 2), -1, np.int32)
    lens = np.zeros((m, max_paths), np.int32)
    status = np.zeros(m, np.int32)
    for k in range(m):
        if counts[k] > cap:
            status[k] = 1
            continue
        keys = keys_of(points[k], max(int(counts[k]), 0))
        for r, path in enumerate(_paths(keys, min_nb_nodes, max_paths)):
            if nb_points is not None and nb_points > 0:
                path = [path[i] for i in resample_indices(len(path), nb_points)]
            if len(path) > slot:
                status[k] = 2
                continue
            xy = np.array([(keys[i] & 0xffff, keys[i] >> 16) for i in path], np.int32)
            nodes[k, r, :len(path)] = xy
            nodes[k, r, len(path):] = xy[-1]
            lens[k, r] = len(path)
    return nodes, lens, status


def hand_shapes():
    """The hand-made units of the tests: [(name, [(y, x), ...] in raster order, dict(min_nb_nodes, max_paths))], all on a map of
    65535 x 40 (the kernel reads coordinates from the points alone)."""
    W = 40
    row = lambda y, x0, x1: [(y, x) for x in range(x0, x1 + 1)]
    col = lambda x, y0, y1: [(y, x) for y in range(y0, y1 + 1)]
    shapes = [
        ("empty", [], {}),
        ("one pixel", [(3, 4)], {}),
        ("chain of min_nb_nodes - 1", row(5, 2, 4), {}),
        ("chain of min_nb_nodes", row(5, 2, 5), {}),
        ("one pixel, min_nb_nodes 1", [(3, 4)], dict(min_nb_nodes=1)),
        ("L", col(3, 2, 7) + row(7, 4, 8), {}),
        ("T", row(2, 1, 9) + col(5, 3, 7), {}),
        ("Y", [(0, 0), (1, 1), (2, 2), (0, 4), (1, 3), (3, 2), (4, 2), (5, 2)], {}),
        ("plus", row(5, 1, 9) + col(5, 1, 4) + col(5, 6, 9), {}),
        ("ring", [(0, 2), (1, 1), (1, 3), (2, 0), (2, 4), (3, 1), (3, 3), (4, 2)], {}),
        ("square ring", row(2, 2, 6) + row(6, 2, 6) + col(2, 3, 5) + col(6, 3, 5), {}),
        ("3 x 3 block", row(1, 1, 3) + row(2, 1, 3) + row(3, 1, 3), {}),
        ("two components of equal length", row(6, 10, 14) + row(2, 3, 7), {}),
        ("three components, max_paths 2", row(1, 1, 4) + row(4, 1, 6) + row(7, 1, 5), {}),
        ("three components, max_paths 8", row(1, 1, 4) + row(4, 1, 6) + row(7, 1, 5), dict(max_paths=8)),
        ("map corner and edges", row(0, 0, W - 1) + col(W - 1, 1, 6) + col(0, 1, 3), {}),
        ("last row of the map", row(65534, 30, W - 1) + col(W - 1, 65528, 65533), {}),
        ("diagonal through y = 32768", [(32760 + i, 10 + i) for i in range(17)], {}),
        ("row end and next row start", row(3, W - 4, W - 1) + row(4, 0, 3), {}),
    ]
    return [(name, sorted(pix), kw) for name, pix, kw in shapes], (65535, W)


def points_of_pixels(pixels, cap):
    """int32 [cap] = (y << 16) | x of raster-ordered pixels, the tail filled with -1 (which the kernel must not read)."""
    out = np.full(cap, -1, np.int32)
    out[:len(pixels)] = np.array([(y << 16) | x for y, x in pixels], np.int64).astype(np.uint32).view(np.int32) if pixels else []
    return out
