"""The error-driven scribble robot (``csrc/robot.hip``): scribbles where the segmentation is wrong.  For every object of the annotated frame
the device thins the error region ``gt == o and pred != o`` to a skeleton - one workgroup per (frame, object) unit, one launch - and the
few hundred skeleton pixels that come back become paths in davisinteractive's schema on the host.

davisinteractive's ``InteractiveScribblesRobot`` does the same on the CPU with skimage's skeletoniser at every interaction of every
episode.  Neither package is a dependency of this one and the robot is not in the reference tree: the rules - Zhang-Suen thinning as
published, the component / double-BFS / resampling step below - are stated in ``include/ivosw.h`` and, as numpy, in ``tests/robot_ref.py``.
They are this project's DEFINITION; parity with the library's own robot is restated, not recorded.

Two entries, the same bits.  A size whose two full-frame bit planes fit the LDS of one workgroup (``fits``: 480 x 854 does) goes to
``ivosw_robot_skeleton`` as long as no unit names object 0.  Every other call - 720p, 1080p, any size up to 65535 x 65535, and the
background - goes to ``ivosw_robot_skeleton_box``, which keeps planes of the error region's bounding box only: in LDS when the box fits,
else in a cached device workspace.  The background (object 0) is drawn on the false positives ``gt == 0 and pred != 0``, as the library's
robot draws it; ``interact(..., background=True)`` asks for it.

There is no CPU fallback for ``skeleton_points``; ``paths_from_points`` is host work.  ``paths_device`` is the same path step on the
device (``csrc/robot_paths.hip``: ``ivosw_robot_paths``, bit for bit the same paths), ``interact_device`` and ``interact_maps`` chain it
behind the skeleton - and in front of ``ivosw_scribble_raster`` - without a copy or a synchronisation; ``interact(paths="device")`` opts in.
"""
import numpy as np
import torch

from .. import _lib as L

# P2 .. P9 of the thinning rule, and the order in which the BFS visits a node's neighbours: N, NE, E, SE, S, SW, W, NW as (dy, dx)
NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def fits(size):
    """Whether maps of ``size`` = (H, W) fit the kernel's two LDS bit planes (``ivosw_robot_skeleton_fits``)."""
    H, W = (int(v) for v in size)
    return bool(L.lib().ivosw_robot_skeleton_fits(H, W))


def _label_map(t, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"robot: {who} must be a device tensor: the skeleton is built on the MI355X only (no CPU fallback)")
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise TypeError(f"robot: {who} must be a uint8 label map [n,H,W], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _launch(gt, pred, units, cap, want_bits):
    """(buffer int32 [m * (2 + cap)] = [counts | iters | points], m, bit planes or None)."""
    gt = _label_map(gt, "gt")
    if pred is not None:
        pred = _label_map(pred, "pred")
        if pred.shape != gt.shape or pred.device != gt.device:
            raise ValueError(f"robot: pred {tuple(pred.shape)} on {pred.device} does not match gt {tuple(gt.shape)} on {gt.device}")
    table = np.ascontiguousarray(np.asarray(units, dtype=np.int32).reshape(-1, 2))
    m, cap = len(table), int(cap)
    n, H, W = gt.shape
    buf = torch.empty(m * (2 + max(cap, 0)), dtype=torch.int32, device=gt.device)
    bits = torch.empty((m, H, (W + 31) // 32), dtype=torch.int32, device=gt.device) if want_bits else None
    lib = L.lib()
    args = (L.dptr(gt), None if pred is None else L.dptr(pred), n, H, W, table.ctypes.data, m, cap,
            L.torch_ptr(buf, 2 * m), L.dptr(buf), L.torch_ptr(buf, m), None if bits is None else L.dptr(bits))
    if lib.ivosw_robot_skeleton_fits(H, W) and not (table[:, 1] == 0).any():
        L.check(lib.ivosw_robot_skeleton(*args, L.stream_ptr(gt.device)), "robot_skeleton")
        return buf, m, bits
    need = max(int(lib.ivosw_robot_box_workspace_bytes(H, W, max(m, 1))), 0)       # (a refused size: the entry says why)
    ws = _workspace(gt.device, need) if need else None
    L.check(lib.ivosw_robot_skeleton_box(*args, None if ws is None else L.dptr(ws), need, L.stream_ptr(gt.device)), "robot_skeleton_box")
    return buf, m, bits


_ws = {}                      # (device, bytes) -> uint8 tensor: the global planes of boxes beyond LDS (calls on one stream are ordered)


def _workspace(device, nbytes):
    key = (torch.device(device), int(nbytes))
    if key not in _ws:
        _ws[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return _ws[key]


def skeleton_points(gt, pred, units, cap=4096, want_bits=False):
    """``ivosw_robot_skeleton`` (a size that ``fits``, no object 0) or ``ivosw_robot_skeleton_box`` (any other call; the same bits) on
    device label maps ``gt`` and ``pred`` (uint8 [n,H,W]; ``pred`` None: all background, no unit of object 0 then) for ``units`` =
    [(frame, object), ...]: device tensors ``(points, counts, iters)`` - int32 [m,cap] skeleton pixels as (y << 16) | x in raster order,
    int32 [m] true pixel counts (also beyond ``cap``) and int32 [m] iteration counts (-1: not converged) - and, ``want_bits``, the
    skeleton's bit planes [m,H,ceil(W/32)] as a fourth (bit x & 31 of word x >> 5; an int32 tensor holding the uint32 words).  The three
    are views of ONE buffer, so a single copy brings them to the host.  One launch per 64 units, no synchronisation."""
    buf, m, bits = _launch(gt, pred, units, cap, want_bits)
    points, counts, iters = buf[2 * m:].view(m, int(cap)), buf[:m], buf[m:2 * m]
    return (points, counts, iters, bits) if want_bits else (points, counts, iters)


def _components(pixels):
    """8-connected components of a raster-ordered list of (y, x): raster-ordered lists, in the order of their first pixels."""
    index = {p: i for i, p in enumerate(pixels)}
    seen = np.zeros(len(pixels), bool)
    comps = []
    for i, p in enumerate(pixels):
        if seen[i]:
            continue
        seen[i] = True
        stack, members = [p], []
        while stack:
            y, x = stack.pop()
            members.append((y, x))
            for dy, dx in NEIGHBOURS:
                j = index.get((y + dy, x + dx))
                if j is not None and not seen[j]:
                    seen[j] = True
                    stack.append((y + dy, x + dx))
        members.sort()
        comps.append(members)
    return comps


def _bfs(inside, start):
    dist, parent, queue = {start: 0}, {start: None}, [start]
    for y, x in queue:                                            # (the list grows while it is walked)
        d = dist[(y, x)] + 1
        for dy, dx in NEIGHBOURS:
            q = (y + dy, x + dx)
            if q in inside and q not in dist:
                dist[q], parent[q] = d, (y, x)
                queue.append(q)
    return dist, parent


def _farthest(dist):
    best = max(dist.values())
    return min(p for p, d in dist.items() if d == best)           # ties: the lower raster index


def longest_paths(pixels, min_nb_nodes=4, max_paths=2):
    """The paths before resampling, as lists of (y, x) nodes.  ``pixels``: skeleton pixels (y, x) in raster order.  Components of fewer
    than ``min_nb_nodes`` pixels are dropped; per component a longest shortest path by double BFS (from the component's first pixel to
    the farthest node a, from a to the farthest node b; neighbours in the order N, NE, E, SE, S, SW, W, NW, a tie between farthest
    nodes goes to the lower raster index; the path runs from a to b); the ``max_paths`` longest are kept, longest first, ties to the
    component with the lower first pixel."""
    paths = []
    for members in _components(pixels):
        if len(members) < int(min_nb_nodes):
            continue
        inside = set(members)
        a = _farthest(_bfs(inside, members[0])[0])
        dist, parent = _bfs(inside, a)
        node, path = _farthest(dist), []
        while node is not None:
            path.append(node)
            node = parent[node]
        paths.append(path[::-1])
    order = sorted(range(len(paths)), key=lambda k: (-len(paths[k]), k))
    return [paths[k] for k in order[:int(max_paths)]]


def paths_from_points(points, count, size, object_id, min_nb_nodes=4, max_paths=2, nb_points=8):
    """The paths of one unit from its skeleton pixels ``points`` (host int32 [cap], (y << 16) | x in raster order, ``count`` of them
    valid) on maps of ``size`` = (H, W): ``longest_paths``, each thinned to at most ``nb_points`` nodes (``np.linspace`` over the node
    indices, rounded, duplicates dropped - ``entry.robot_paths``' rule; None keeps every node, so that the polyline stays on the
    skeleton) and emitted as ``dict(path=[[(x + 0.5) / W, (y + 0.5) / H], ...], object_id=o, start_time=0, end_time=0)``.
    ``count`` above ``len(points)`` (the skeleton did not fit the cap) is a ValueError."""
    H, W = (int(v) for v in size)
    points, count = np.asarray(points).reshape(-1), int(count)
    if count > len(points):
        raise ValueError(f"robot: object {object_id}: the skeleton has {count} pixels, more than the cap of {len(points)} points")
    v = points[:count].astype(np.int64) & 0xffffffff
    pixels = list(zip((v >> 16).tolist(), (v & 0xffff).tolist()))
    out = []
    for path in longest_paths(pixels, min_nb_nodes, max_paths):
        if nb_points is not None:
            idx = np.unique(np.linspace(0, len(path) - 1, min(int(nb_points), len(path))).round().astype(int))
            path = [path[i] for i in idx]
        out.append(dict(path=[[(x + 0.5) / W, (y + 0.5) / H] for y, x in path], object_id=int(object_id), start_time=0, end_time=0))
    return out


class DevicePaths:
    """The outputs of ``ivosw_robot_paths`` for m units: ``nodes`` int32 [m,max_paths,slot,2] = (x, y), ``lens`` int32 [m,max_paths] and
    ``status`` int32 [m], three views of ONE device buffer [nodes | lens | status], so that one copy brings them home.  ``objects``: the
    object id of every unit; ``size`` = (H, W) of the maps the nodes lie on; ``counts``: the skeleton's device counts (read only to word a
    refusal)."""

    def __init__(self, buf, objects, size, max_paths, slot, cap, counts=None, frame=None):
        self.buf, self.objects, self.size = buf, [int(o) for o in objects], tuple(int(v) for v in size)
        self.max_paths, self.slot, self.cap, self.counts, self.frame = int(max_paths), int(slot), int(cap), counts, frame
        m, n = len(self.objects), len(self.objects) * self.max_paths * self.slot * 2
        self.nodes = buf[:n].view(m, self.max_paths, self.slot, 2)
        self.lens = buf[n:n + m * self.max_paths].view(m, self.max_paths)
        self.status = buf[n + m * self.max_paths:]

    def to_scribbles(self):
        """The one copy (and the one synchronisation): the list ``interact`` returns - the same dicts, the same floats, the same order.
        A unit whose skeleton did not fit the cap (status 1) is the ValueError of ``interact``; a path longer than ``slot`` (status 2) is
        a ValueError that names ``slot``."""
        m = len(self.objects)
        if m == 0:
            return []
        flat = self.buf.cpu().numpy()
        H, W = self.size
        n = m * self.max_paths * self.slot * 2
        nodes, lens, status = flat[:n].reshape(m, self.max_paths, self.slot, 2), flat[n:n + m * self.max_paths].reshape(m, -1), flat[n + m * self.max_paths:]
        out = []
        for k, o in enumerate(self.objects):
            if status[k] == 1:
                count = "" if self.counts is None else f" {int(self.counts[k])}"
                where = f"object {o}" if self.frame is None else f"frame {self.frame}, object {o}"
                raise ValueError(f"robot: unit {k} ({where}): the skeleton has{count} pixels, more than cap = {self.cap}")
            if status[k] == 2:
                raise ValueError(f"robot: unit {k} (object {o}): a path has more nodes than slot = {self.slot} (nb_points=None keeps every "
                                 f"node: give a larger slot, at most cap = {self.cap})")
            for r in range(self.max_paths):
                if lens[k, r] > 0:
                    out.append(dict(path=[[(x + 0.5) / W, (y + 0.5) / H] for x, y in nodes[k, r, :lens[k, r]].tolist()], object_id=o,
                                    start_time=0, end_time=0))
        return out

    def table(self, map_index=0):
        """The static host table of ``ivosw_scribble_raster`` over ``nodes`` as its point array: int32 [m * max_paths, 4] =
        {(k * max_paths + r) * slot, slot, object_k, map_index}.  A slot behind its path repeats the last node (zero-length segments: the
        same pixel under the same path index) and a slot without a path holds (-1, -1), which the draw kernel does not draw."""
        rows = [((k * self.max_paths + r) * self.slot, self.slot, o, int(map_index)) for k, o in enumerate(self.objects)
                for r in range(self.max_paths)]
        return np.array(rows, dtype=np.int32).reshape(-1, 4)


def paths_device(points, counts, objects, size, min_nb_nodes=4, max_paths=2, nb_points=8, slot=None):
    """``ivosw_robot_paths`` on the device tensors ``skeleton_points`` returns (``points`` int32 [m,cap], ``counts`` int32 [m]) for units of
    the objects ``objects`` on maps of ``size`` = (H, W): a ``DevicePaths``.  ``nb_points`` None keeps every node.  ``slot``: the entries
    per path (None: ``nb_points``, or ``cap`` when every node is kept).  One launch per 64 units, no copy, no synchronisation."""
    H, W = (int(v) for v in size)
    m, cap = points.shape
    objects = [int(o) for o in objects]
    if len(objects) != m or counts.numel() != m:
        raise ValueError(f"robot: {m} units of points, {counts.numel()} counts and {len(objects)} objects")
    nb = 0 if nb_points is None else int(nb_points)
    if nb_points is not None and nb < 1:
        raise ValueError(f"robot: nb_points must be None or >= 1, got {nb_points!r}")
    slot = (nb if nb > 0 else cap) if slot is None else int(slot)
    max_paths = int(max_paths)
    buf = torch.empty(m * max(max_paths, 0) * max(slot, 0) * 2 + m * max(max_paths, 0) + m, dtype=torch.int32, device=points.device)
    n = m * max_paths * slot * 2
    L.check(L.lib().ivosw_robot_paths(L.dptr(points, torch.int32), L.dptr(counts, torch.int32), m, cap, H, W, int(min_nb_nodes), max_paths, nb,
                                      slot, L.dptr(buf), L.torch_ptr(buf, max(n, 0)), L.torch_ptr(buf, max(n, 0) + m * max(max_paths, 0)),
                                      L.stream_ptr(points.device)), "robot_paths")
    return DevicePaths(buf, objects, (H, W), max_paths, slot, cap, counts)


def interact_device(gt, pred, n_objects, frame, cap=4096, background=False, **kw):
    """``interact`` without leaving the device: skeleton -> paths, two launches, no copy, no synchronisation.  A ``DevicePaths`` whose
    ``to_scribbles()`` is the list ``interact`` returns; ``kw``: ``min_nb_nodes``, ``max_paths``, ``nb_points``, ``slot`` of
    ``paths_device``."""
    frame, n_objects = int(frame), int(n_objects)
    if n_objects < 1:
        return DevicePaths(torch.empty(0, dtype=torch.int32, device=gt.device), [], gt.shape[1:], kw.get("max_paths", 2), 1, cap)
    units = [(frame, o) for o in range(0 if background and pred is not None else 1, n_objects + 1)]
    buf, m, _ = _launch(gt, pred, units, cap, False)
    out = paths_device(buf[2 * m:].view(m, int(cap)), buf[:m], [o for _, o in units], gt.shape[1:], **kw)
    out.frame = frame
    return out


def maps_from_paths(paths, size=None, default_value=-1, roi_dist=None, as_float=False):
    """The scribble map [1,h,w] of a ``DevicePaths`` drawn by ``ivosw_scribble_raster`` straight from the device nodes: only the static
    table is uploaded.  ``size`` None or the paths' own size: the nodes as they are ((x + 0.5) / W packs back to x exactly).  Another
    ``size`` = (h, w): every node is scaled with ``scribbles.pack``'s own expression in float64 on the device, px = min(int((x + 0.5) / W
    * w), w - 1) (a few elementwise tensor operations on the node array; (-1, -1) stays (-1, -1)), so the map is that of ``scribble_maps``
    on the host paths at that size.  No synchronisation."""
    from . import scribbles as S
    H, W = paths.size
    h, w = (H, W) if size is None else (int(v) for v in size)
    m = len(paths.objects)
    if m == 0:
        return S.raster(np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), 1, (h, w), paths.buf.device, default_value, roi_dist, as_float)
    nodes = paths.nodes
    if (h, w) != (H, W):
        v = nodes.to(torch.float64)
        scaled = torch.stack([torch.clamp(((v[..., 0] + 0.5) / W * w).to(torch.int32), max=w - 1),
                              torch.clamp(((v[..., 1] + 0.5) / H * h).to(torch.int32), max=h - 1)], -1)
        nodes = torch.where(nodes < 0, nodes, scaled).contiguous()
    return S.raster_device(nodes, paths.table(0), 1, (h, w), default_value, roi_dist, as_float)


def interact_maps(gt, pred, n_objects, frame, size=None, default_value=-1, roi_dist=None, as_float=False, **kw):
    """skeleton -> paths -> raster with no synchronisation: ``(maps, DevicePaths)``, ``maps`` a device int8 (``as_float``: float32)
    [1,h,w].  With ``size`` None or the frame size, ``maps`` is ``scribble_maps({"scribbles": [interact(...)]}, size)`` bit for bit
    whenever ``interact`` draws a path at all (without one ``scribble_maps`` returns no map; this returns one map of ``default_value``).
    Another ``size`` is served too: see ``maps_from_paths``.  ``kw``: ``cap``, ``background`` and the keywords of ``paths_device``."""
    paths = interact_device(gt, pred, n_objects, frame, **kw)
    return maps_from_paths(paths, size, default_value, roi_dist, as_float), paths


def interact(gt, pred, n_objects, frame, cap=4096, background=False, paths="host", **kw):
    """The scribbles of one frame in davisinteractive's schema: a list of paths for the objects 1 .. ``n_objects`` in ascending order, drawn
    along the skeleton of each object's error region on ``frame``.  ``gt`` and ``pred``: device uint8 [n,H,W] (``pred`` None: nothing
    predicted yet, the error region is the object).  An object without an error skeleton of at least ``min_nb_nodes`` connected pixels
    gets no path.  ``background``: the background is scribbled too - unit (frame, 0), the false positives ``gt == 0 and pred != 0``; its
    paths carry ``object_id=0`` and come first, so the list stays ascending in object id.  With ``pred`` None nothing is predicted, no
    false positive exists and the background is skipped.  ``kw``: ``min_nb_nodes``, ``max_paths``, ``nb_points`` of
    ``paths_from_points``.  One launch, one device-to-host copy of [counts | iters | points], then the numpy step.  ``paths="device"``:
    the path step runs on the device too (``interact_device(...).to_scribbles()``: two launches, one copy of the finished paths; the same
    list); any other value is a ValueError."""
    if paths not in ("host", "device"):
        raise ValueError(f"robot: paths must be 'host' or 'device', got {paths!r}")
    if paths == "device":
        return interact_device(gt, pred, n_objects, frame, cap, background, **kw).to_scribbles()
    frame, n_objects = int(frame), int(n_objects)
    if n_objects < 1:
        return []
    units = [(frame, o) for o in range(0 if background and pred is not None else 1, n_objects + 1)]
    buf, m, _ = _launch(gt, pred, units, cap, False)
    flat = buf.cpu().numpy()                                      # the one copy (and the one synchronisation)
    counts_h, points_h = flat[:m], flat[2 * m:].reshape(m, -1)
    H, W = gt.shape[1:]
    out = []
    for k, (f, o) in enumerate(units):
        if counts_h[k] > points_h.shape[1]:
            raise ValueError(f"robot: unit {k} (frame {f}, object {o}): the skeleton has {int(counts_h[k])} pixels, more than cap = "
                             f"{points_h.shape[1]}")
        out += paths_from_points(points_h[k], counts_h[k], (H, W), o, **kw)
    return out
