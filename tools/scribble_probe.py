"""The scribble chains on the device (ivosw_scribble_raster, ivosw_rough_roi, ivosw_ipn_dilate) against the host sequences they replace
(GPU only).  Robot-like scribbles: one annotated frame of a 100-frame session, 3 objects, 5 paths of 60 points each.

  MANet, 120 x 214   device: utils_manet.scribble_label (pack, one small upload, one memset, two launches, rough_ROI fused), first and
                     later interactions.  replaced: scribbles2mask over all 100 frames into an int64 [100,H,W] host array, the slice,
                     float32, the upload, and - first interaction - rough_ROI as torch calls on the device (nonzero / min / max and the
                     Python slice bounds: a synchronisation), eval_agent_manet.py:368-374.
  IPN, 480 x 854     device: utils_ipn.scribble_input (the raster, then ivosw_ipn_dilate).  replaced: scribbles2mask into an int64
                     [100,H,W] host array (328 MB), the slice, Dilate_mask's per-object loop on the host (scipy's binary_dilation in
                     cv2's place: cv2 is no dependency), the upload.
  calls              the device chains alone, HIP events around 50 calls (host packing included: it is part of every call).

The replaced side's rasteriser is the numpy RESTATEMENT of tests/scribble_ref.py, not davisinteractive's own code: the library is not
installed where this runs, so its own time was not measured.  Host clock around work that ends in a synchronise, the two sides
alternating in one process, medians and min .. max over 5 rounds.

usage: python tools/scribble_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, T, FRAME, N_OBJECTS, N_PATHS, N_POINTS = 5, 100, 40, 3, 5, 60


def _events(fn, n, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / n                # us per call


def _wall(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3             # ms


def _alternate(legs, measure, warm):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            out[k].append(measure(fn))
    return out


def _fmt(v, unit):
    return f"{statistics.median(v):9.2f} {unit}  ({min(v):.2f} .. {max(v):.2f})"


def robot_scribbles(seed=7):
    """One annotated frame: N_PATHS random walks of N_POINTS points (steps of about 1 % of the frame) over N_OBJECTS objects."""
    import numpy as np
    rng = np.random.default_rng(seed)
    paths = []
    for k in range(N_PATHS):
        walk = np.clip(np.cumsum(np.vstack([rng.uniform(0.2, 0.8, (1, 2)), rng.normal(0, 0.01, (N_POINTS - 1, 2))]), 0), 0.0, 1.0)
        paths.append(dict(path=walk.tolist(), object_id=1 + k % N_OBJECTS, start_time=0, end_time=0))
    return dict(sequence="probe", scribbles=[paths if f == FRAME else [] for f in range(T)])


def host_rough_roi(lab, dist=20):
    """rough_ROI's rule as torch calls on the tensor's device, with the synchronisation its Python slice bounds need."""
    import torch
    h, w = lab.shape[-2:]
    nz = (lab[0, 0] != -1).nonzero()
    (h_min, w_min), (h_max, w_max) = nz.min(0)[0].tolist(), nz.max(0)[0].tolist()
    r0, r1, c0, c1 = max(h_min - dist, 0), min(h_max + dist, h - 1), max(w_min - dist, 0), min(w_max + dist, w - 1)
    out = torch.zeros_like(lab)
    out[..., r0:r1, c0:c1] = lab[..., r0:r1, c0:c1]
    return out


def host_dilate(mask, num_objects):
    """Dilate_mask's loop with scipy's dilation in cv2's place."""
    import numpy as np
    from scipy import ndimage
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    new_mask = -np.ones_like(mask, dtype=np.int64)
    for o in range(num_objects + 1):
        new_mask[ndimage.binary_dilation(mask == o, structure=cross, iterations=2)] = o
    return new_mask


def main():
    import numpy as np
    import torch
    from ivos_w_amd.utils import scribbles as S
    from ivos_w_amd.utils import utils_ipn, utils_manet
    from tests import scribble_ref as sr
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    sc = robot_scribbles()
    points, table, _ = S.pack(sc, (480, 854))
    print(f"scribble probe: {T} frames, frame {FRAME} annotated, {len(table)} paths, {len(points)} points, {ROUNDS} rounds, medians (min .. max)")
    keep = {}

    # ---- MANet, 120 x 214
    h, w = 120, 214
    for first in (True, False):
        def device_chain():
            keep["a"] = utils_manet.scribble_label(sc, FRAME, (h, w), first, dev)

        def replaced():
            masks = sr.scribbles2mask(sc, (h, w), dtype=np.int64)
            lab = torch.from_numpy(masks[FRAME].astype(np.float32))[None, None].to(dev)
            keep["b"] = host_rough_roi(lab) if first else lab

        r = _alternate({"device": device_chain, "replaced": replaced}, lambda fn: _wall(fn, dev), 2)
        assert torch.equal(keep["a"], keep["b"])
        what = "first interaction (rough_ROI)" if first else "later interaction"
        print(f"MANet {h} x {w}, {what}:  device chain {_fmt(r['device'], 'ms')}   host sequence {_fmt(r['replaced'], 'ms')}")
        d = [_events(device_chain, 50, dev) for _ in range(ROUNDS)]
        print(f"    scribble_label alone, HIP events over 50 calls: {_fmt(d, 'us')} per call")

    # ---- IPN, 480 x 854
    h, w = 480, 854

    def device_chain():
        keep["a"] = utils_ipn.scribble_input(sc, FRAME, (h, w), N_OBJECTS, dev)

    def replaced():
        masks = sr.scribbles2mask(sc, (h, w), dtype=np.int64)
        keep["b"] = torch.from_numpy(host_dilate(masks[FRAME], N_OBJECTS)).to(dev)

    r = _alternate({"device": device_chain, "replaced": replaced}, lambda fn: _wall(fn, dev), 2)
    assert torch.equal(keep["a"].long(), keep["b"])
    print(f"IPN {h} x {w} (raster + dilation):  device chain {_fmt(r['device'], 'ms')}   host sequence {_fmt(r['replaced'], 'ms')}")
    print(f"    the host sequence allocates an int64 [{T},{h},{w}] array of {T * h * w * 8 / 1e6:.0f} MB per call; the device chain uploads "
          f"{(points.nbytes + table.nbytes) / 1e3:.1f} KB")
    d = [_events(device_chain, 50, dev) for _ in range(ROUNDS)]
    print(f"    scribble_input alone, HIP events over 50 calls: {_fmt(d, 'us')} per call")
    t0 = time.perf_counter()
    for _ in range(200):
        S.pack(sc, (h, w), [FRAME])
    print(f"    of which host packing (numpy, {len(points)} points): {(time.perf_counter() - t0) / 200 * 1e6:.0f} us per call")


if __name__ == "__main__":
    main()
