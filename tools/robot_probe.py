"""The error-driven scribble robot on the device (ivosw_robot_skeleton, utils/robot.py) against a host robot (GPU only), 480 x 854.

  interact     utils.robot.interact for 1 and 3 objects: one launch, one copy back of [counts | iters | points], the numpy path step.
               host: the label maps copied back (the robot the library ships is host code: it needs them there), per object the
               vectorised numpy Zhang-Suen of tests/robot_ref.py (thin_fast: the rule tabulated over the 256 neighbourhoods, every pixel of a
               sub-iteration in one expression) and the SAME path step.  Two error regions per object: thick (a disc of radius about 100
               that the prediction misses altogether) and thin (the prediction is the ground truth moved by 2 pixels: a sliver along the
               boundary).
  kernel       ivosw_robot_skeleton alone per unit, HIP events around 20 calls, with the iteration count it reports.

The host side is this project's RESTATEMENT of the rule, not davisinteractive's robot (skimage's skeletoniser, networkx paths): neither
package is installed where this runs, so the library's own time was not measured.  Host clock around work that ends in a synchronise, the
two sides alternating in one process, medians and min .. max over 5 rounds.

usage: python tools/robot_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, H, W, FRAME = 5, 480, 854, 1


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


def scene(n_objects, kind):
    """(gt, pred) uint8 [2,H,W]: discs of radius 100, 90 and 80 as objects 1 .. n_objects on frame FRAME; ``thick``: nothing of them is
    predicted, ``thin``: the prediction is the ground truth moved by 2 pixels in x and y."""
    import numpy as np
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((2, H, W), np.uint8)
    for o, (cy, cx, r) in enumerate([(240, 150, 100), (130, 420, 90), (350, 700, 80)][:n_objects], 1):
        gt[FRAME][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = o
    pred = np.zeros_like(gt) if kind == "thick" else np.roll(gt, (2, 2), (1, 2))
    return gt, pred


def main():
    import numpy as np
    import torch
    from ivos_w_amd.utils import robot as R
    from tests import robot_ref as rr
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    print(f"robot probe: {H} x {W}, {ROUNDS} rounds, medians (min .. max); host side = numpy restatement (tests/robot_ref.thin_fast), "
          "NOT davisinteractive's robot")
    keep = {}
    for kind in ("thick", "thin"):
        for n_objects in (1, 3):
            gt, pred = scene(n_objects, kind)
            d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)

            def device_side():
                keep["a"] = R.interact(d_gt, d_pred, n_objects, FRAME)

            def host_side():
                g, p = d_gt[FRAME].cpu().numpy(), d_pred[FRAME].cpu().numpy()
                out = []
                for o in range(1, n_objects + 1):
                    sk, _ = rr.thin_fast(rr.error_plane(g, p, o))
                    pts = rr.points_of(sk)
                    out += R.paths_from_points(pts, len(pts), (H, W), o)
                keep["b"] = out

            r = _alternate({"device": device_side, "host": host_side}, lambda fn: _wall(fn, dev), 1)
            assert keep["a"] == keep["b"], "the two robots disagree"
            units = [(FRAME, o) for o in range(1, n_objects + 1)]
            points, counts, iters = R.skeleton_points(d_gt, d_pred, units)
            torch.cuda.synchronize(dev)
            k = [_events(lambda: R.skeleton_points(d_gt, d_pred, units), 20, dev) for _ in range(ROUNDS)]
            print(f"{kind:5s} error region, {n_objects} object(s): {len(keep['a'])} paths, skeleton pixels {counts.tolist()}, iterations {iters.tolist()}")
            print(f"    interact          device {_fmt(r['device'], 'ms')}   host {_fmt(r['host'], 'ms')}   "
                  f"ratio of medians {statistics.median(r['host']) / statistics.median(r['device']):.1f} x")
            print(f"    kernel alone      {_fmt(k, 'us')} per call of {n_objects} unit(s) (one workgroup each, HIP events over 20 calls)")
            path_ms = []
            pts_h, cnt_h = points.cpu().numpy(), counts.cpu().numpy()
            for _ in range(ROUNDS):
                t0 = time.perf_counter()
                for j, (_, o) in enumerate(units):
                    R.paths_from_points(pts_h[j], cnt_h[j], (H, W), o)
                path_ms.append((time.perf_counter() - t0) * 1e3)
            print(f"    of which the numpy path step (both sides run it): {_fmt(path_ms, 'ms')}")


if __name__ == "__main__":
    main()
