"""The robot's path step on the device (ivosw_robot_paths, utils/robot.py) against the numpy path step (GPU only), 480 x 854.

  cases        the two scenes of tools/robot_probe.py (thick: discs the prediction misses altogether; thin: the prediction is the ground
               truth moved by 2 pixels) for 1 and 3 objects, and one unit whose skeleton FILLS the cap: a chain of 4096 pixels winding
               through the frame (about 2 x 4096 dependent BFS levels of one node each - the worst case of a level-synchronous sweep).
  interact     utils.robot.interact with paths="host" against paths="device", host clock around calls that end in their copy.
  maps         utils.robot.interact_maps (skeleton -> paths -> raster, then a synchronise) against the host sequence interact +
               scribbles.scribble_maps.
  kernel       ivosw_robot_paths alone on the skeleton's device outputs, HIP events around 20 calls, for the workgroup widths 64, 256 and
               1024 (tunable RPATHS_T; the library's default is 64).
The legs alternate in one process; medians and min .. max over 5 rounds.  Both legs of every pair are checked to agree.

usage: python tools/robot_paths_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from robot_probe import FRAME, H, ROUNDS, W, _alternate, _events, _fmt, _wall, scene      # noqa: E402

CAP = 4096


def chain_scene():
    """(gt, pred): object 1 is a one-pixel-wide chain of exactly CAP pixels (rows of W - 2 pixels on every other row, joined by single
    pixels diagonally outside the row ends), nothing predicted: thinning keeps it whole, so the skeleton fills the cap."""
    import numpy as np
    gt = np.zeros((2, H, W), np.uint8)
    n, y, right = 0, 0, True
    while n < CAP:
        k = min(W - 2, CAP - n)
        xs = np.arange(1, W - 1) if right else np.arange(W - 2, 0, -1)
        gt[FRAME, y, xs[:k]] = 1
        n += k
        if n < CAP:
            gt[FRAME, y + 1, W - 1 if right else 0] = 1
            n += 1
        y, right = y + 2, not right
    return gt, np.zeros_like(gt)


def main():
    import torch
    from ivos_w_amd import _lib as L
    from ivos_w_amd.utils import robot as R
    from ivos_w_amd.utils import scribbles as S
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    print(f"robot paths probe: {H} x {W}, cap {CAP}, {ROUNDS} rounds, medians (min .. max); nb_points 8, max_paths 2, min_nb_nodes 4")
    keep = {}
    cases = [(f"{kind} error region, {n} object(s)", n, scene(n, kind)) for kind in ("thick", "thin") for n in (1, 3)]
    cases.append(("a chain that fills the cap, 1 object", 1, chain_scene()))
    for name, n_objects, (gt, pred) in cases:
        d_gt, d_pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)

        def host_paths():
            keep["h"] = R.interact(d_gt, d_pred, n_objects, FRAME, cap=CAP)

        def device_paths():
            keep["d"] = R.interact(d_gt, d_pred, n_objects, FRAME, cap=CAP, paths="device")

        def host_maps():
            keep["hm"] = S.scribble_maps({"scribbles": [R.interact(d_gt, d_pred, n_objects, FRAME, cap=CAP)]}, (H, W), frames=[0],
                                         device=dev)              # (frames: one map also when no path was drawn)

        def device_maps():
            keep["dm"] = R.interact_maps(d_gt, d_pred, n_objects, FRAME, cap=CAP)[0]

        r = _alternate({"host": host_paths, "device": device_paths}, lambda fn: _wall(fn, dev), 2)
        assert keep["h"] == keep["d"], "the two path steps disagree"
        q = _alternate({"host": host_maps, "device": device_maps}, lambda fn: _wall(fn, dev), 2)
        assert torch.equal(keep["hm"], keep["dm"]), "the two maps disagree"
        units = [(FRAME, o) for o in range(1, n_objects + 1)]
        points, counts, _ = R.skeleton_points(d_gt, d_pred, units, cap=CAP)
        torch.cuda.synchronize(dev)
        print(f"{name}: {len(keep['h'])} paths, skeleton pixels {counts.tolist()}")
        for tag, v in (("interact     ", r), ("interact_maps", q)):
            print(f"    {tag}  host {_fmt(v['host'], 'ms')}   device {_fmt(v['device'], 'ms')}   "
                  f"ratio of medians {statistics.median(v['host']) / statistics.median(v['device']):.2f} x")
        for width in (64, 256, 1024):
            L.tune_set("RPATHS_T", width)
            fn = lambda: R.paths_device(points, counts, [o for _, o in units], (H, W))
            fn()
            k = [_events(fn, 20, dev) for _ in range(ROUNDS)]
            print(f"    kernel alone, {width:4d} threads  {_fmt(k, 'us')} per call of {n_objects} unit(s) (HIP events over 20 calls)")
        L.tune_set("RPATHS_T", 0)


if __name__ == "__main__":
    main()
