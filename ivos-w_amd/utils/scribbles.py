"""Scribbles on the device (``csrc/scribble.hip``): the paths an annotator or the robot has just drawn go up as a few KB of integers and
the label maps are drawn where their consumers read them - MANet's ``scribble_label`` (``utils_manet.scribble_label``), IPN's dilation
(``utils_ipn.scribble_input``) and the overlays.  davisinteractive's ``scribbles2mask`` fills an int64 [n_frames,H,W] host array per call
(328 MB for a 100-frame 480p session) with a Python line loop, although with ``only_last=True`` a single frame has paths at all.

The schema is davisinteractive's: ``scribbles["scribbles"]`` is one list per frame of paths ``dict(path=[[x, y], ...], object_id=o, ...)``
with x and y in [0, 1].  The rules - packing, the line rule, the order of assignment - are stated in ``include/ivosw.h`` and, as numpy, in
``tests/scribble_ref.py``.  They are this project's DEFINITION: davisinteractive is not a dependency of this package and its
``scribbles2mask`` is not in the reference tree, so parity with the library's own rasteriser is restated, not recorded.

There is no CPU fallback for the device entries; ``pack`` is host work.
"""
import numpy as np
import torch

from .. import _lib as L

MAX_OBJECT_ID = 126           # the maps are int8 and -1 is taken (utils_ipn.MAX_OBJECTS)
_ws = {}                      # device -> Workspace (grow-only; calls on one stream are ordered)


def _size(size, who):
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: the map size must be positive, got {(H, W)}")
    return H, W


def pack(scribbles, size, frames=None):
    """The integer points and the path table of ``ivosw_scribble_raster`` for maps of ``size`` = (H, W): ``(points, table, frames)``,
    int32 [P,2] = (px, py), int32 [n_paths,4] = {first point, number of points, object id, map index} and the list of frames - map j is
    frame ``frames[j]``.  ``frames`` None: every frame that has at least one non-empty path, ascending.  Empty paths are skipped.
    px = min(int(x * W), W - 1), py = min(int(y * H), H - 1), the products in float64 and truncated; the clamp of 1.0 to the last pixel
    is this project's rule.  A coordinate outside [0, 1] or not finite is a ValueError that names frame and path."""
    H, W = _size(size, "pack")
    per_frame = scribbles["scribbles"]
    n_frames = len(per_frame)
    if frames is None:
        frames = [f for f in range(n_frames) if any(len(p.get("path", ())) for p in per_frame[f])]
    else:
        frames = [int(f) for f in frames]
        if len(set(frames)) != len(frames) or any(f < 0 or f >= n_frames for f in frames):
            raise ValueError(f"pack: frames must be distinct frames in [0, {n_frames}), got {frames}")
    chunks, rows, first = [], [], 0
    for j, f in enumerate(frames):
        for k, p in enumerate(per_frame[f]):
            if "path" not in p or "object_id" not in p:
                raise ValueError(f"pack: frame {f}, path {k}: a path is dict(path=[[x, y], ...], object_id=o, ...), got keys {sorted(p)}")
            pts = np.asarray(p["path"], dtype=np.float64)
            if pts.size == 0:
                continue
            if pts.ndim != 2 or pts.shape[1] != 2:
                raise ValueError(f"pack: frame {f}, path {k}: a path is a list of [x, y] points, got shape {pts.shape}")
            obj = int(p["object_id"])
            if not 0 <= obj <= MAX_OBJECT_ID:
                raise ValueError(f"pack: frame {f}, path {k}: object_id {obj} outside [0, {MAX_OBJECT_ID}]")
            if not (np.isfinite(pts).all() and (pts >= 0.0).all() and (pts <= 1.0).all()):
                raise ValueError(f"pack: frame {f}, path {k}: a coordinate is outside [0, 1] or not finite")
            chunks.append(pts)
            rows.append((first, len(pts), obj, j))
            first += len(pts)
    if not chunks:
        return np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), frames
    allp = np.concatenate(chunks)
    points = np.minimum((allp * (W, H)).astype(int), (W - 1, H - 1)).astype(np.int32)          # one expression over all points
    return np.ascontiguousarray(points), np.array(rows, dtype=np.int32).reshape(-1, 4), frames


def raster(points, table, n_maps, size, device=None, default_value=-1, roi_dist=None, as_float=False, bresenham=True):
    """``ivosw_scribble_raster`` on packed paths: a device int8 (``as_float``: float32) tensor [n_maps,H,W].  One small upload (points and
    table in one tensor), one memset, two launches, no synchronisation."""
    H, W = _size(size, "raster")
    n_maps = int(n_maps)
    if not torch.cuda.is_available():
        raise RuntimeError("scribbles: the maps are drawn on the MI355X only (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("scribbles: the maps are drawn on the MI355X only (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not -128 <= int(default_value) <= 127:
        raise ValueError(f"scribbles: default_value {default_value} outside int8")
    out = torch.empty((n_maps, H, W), dtype=torch.float32 if as_float else torch.int8, device=dev)
    if n_maps == 0:
        return out
    points = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
    table = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4)
    P, n_paths = len(points), len(table)
    lib = L.lib()
    need = lib.ivosw_scribble_raster_ws_bytes(n_maps, H, W)
    if need == 0:
        raise ValueError(f"scribbles: {n_maps} maps of {H} x {W} are more than 2^31 - 1 pixels")
    ws = _ws.setdefault(dev, L.Workspace()).get(need, dev)
    d_points = d_table = None
    if n_paths:
        both = torch.from_numpy(np.concatenate([points.reshape(-1), table.reshape(-1)])).to(dev, non_blocking=True)
        d_points, d_table = L.dptr(both), L.torch_ptr(both, 2 * P)
    L.check(lib.ivosw_scribble_raster(d_points, P, d_table, table.ctypes.data if n_paths else None, n_paths, n_maps, H, W,
                                      int(default_value), int(bool(bresenham)), -1 if roi_dist is None else int(roi_dist),
                                      None if as_float else L.dptr(out), L.dptr(out) if as_float else None, L.dptr(ws), ws.numel(),
                                      L.stream_ptr(dev)), "scribble_raster")
    return out


def raster_device(d_points, table, n_maps, size, default_value=-1, roi_dist=None, as_float=False, bresenham=True):
    """``raster`` for points that are already on the device: ``d_points`` a contiguous device int32 tensor [..., 2] = (px, py) (the
    ``nodes`` of ``utils.robot.DevicePaths``, for one), ``table`` the host path table over its flattened points.  Only the table is
    uploaded; the maps are drawn on the points' device.  A point outside the map ends the segments it belongs to (the draw kernel's
    rule), so a caller may mark unused points with (-1, -1).  One memset, two launches, no synchronisation."""
    H, W = _size(size, "raster_device")
    n_maps = int(n_maps)
    if not isinstance(d_points, torch.Tensor) or not d_points.is_cuda or d_points.dtype != torch.int32 or d_points.shape[-1:] != (2,):
        raise TypeError("raster_device: d_points must be a device int32 tensor [..., 2]")
    if not -128 <= int(default_value) <= 127:
        raise ValueError(f"scribbles: default_value {default_value} outside int8")
    dev = d_points.device
    out = torch.empty((n_maps, H, W), dtype=torch.float32 if as_float else torch.int8, device=dev)
    if n_maps == 0:
        return out
    table = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4)
    P, n_paths = d_points.numel() // 2, len(table)
    lib = L.lib()
    need = lib.ivosw_scribble_raster_ws_bytes(n_maps, H, W)
    if need == 0:
        raise ValueError(f"scribbles: {n_maps} maps of {H} x {W} are more than 2^31 - 1 pixels")
    ws = _ws.setdefault(dev, L.Workspace()).get(need, dev)
    d_table = torch.from_numpy(table.reshape(-1)).to(dev, non_blocking=True) if n_paths else None
    L.check(lib.ivosw_scribble_raster(L.dptr(d_points) if n_paths else None, P, L.dptr(d_table) if n_paths else None,
                                      table.ctypes.data if n_paths else None, n_paths, n_maps, H, W, int(default_value),
                                      int(bool(bresenham)), -1 if roi_dist is None else int(roi_dist), None if as_float else L.dptr(out),
                                      L.dptr(out) if as_float else None, L.dptr(ws), ws.numel(), L.stream_ptr(dev)), "scribble_raster")
    return out


def scribble_maps(scribbles, size, frames=None, device=None, default_value=-1, roi_dist=None, as_float=False):
    """The label maps of the listed frames only (None: the frames that have paths), a device tensor [m,H,W], int8 or - ``as_float`` -
    float32 with the same values.  ``roi_dist``: apply ``rough_ROI`` with that distance to every map in the same pass (None: off)."""
    points, table, frames = pack(scribbles, size, frames)
    return raster(points, table, len(frames), size, device, default_value, roi_dist, as_float)


def scribbles2mask(scribbles, output_resolution, bezier_curve=False, nb_points=1000, bresenham=True, default_value=-1):
    """davisinteractive's signature; a device int8 [n_frames,H,W] on the current GPU instead of an int64 host array.  The line rule is
    this project's (module docstring).  ``bezier_curve=True`` is refused: the library's curve fit resamples a path into ``nb_points``
    points with scipy, a host step whose parity could not be pinned here - fit the curve before calling if it is wanted."""
    if bezier_curve:
        raise NotImplementedError("scribbles2mask: bezier_curve=True is not rebuilt (the library's Bezier fit resamples the paths on the host "
                                  "and its parity cannot be pinned without the library): pass the resampled paths with bezier_curve=False")
    n_frames = len(scribbles["scribbles"])
    points, table, _ = pack(scribbles, output_resolution, range(n_frames))
    return raster(points, table, n_frames, output_resolution, None, default_value, None, False, bresenham)
