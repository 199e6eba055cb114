"""The boxed error-skeleton entry (ivosw_robot_skeleton_box: planes of the error region's bounding box only) against the full-frame entry
(ivosw_robot_skeleton) and its two plane homes against each other (GPU only).

  480 x 854      a thick region (a missed disc of radius 100) and a thin one (the prediction is the ground truth moved by 2 pixels: a
                 sliver along the boundary): the old entry against the box entry, one unit.
  720p, 1080p    the same two regions through the box entry: the box fits LDS (the old entry refuses these sizes).
  720p, whole    the disc plus one pixel in each of two opposite corners: the box is the whole frame, 230 KB, so the planes live in the
                 global workspace (and every sub-iteration walks 28 800 words instead of the disc's 1 608).
  720p, forced   the disc alone with its planes forced into the workspace (ivosw_robot_box_probe, 256 bytes of LDS) against its LDS
                 window: the same work, the two plane homes.

Every leg is the C entry alone on preallocated buffers, HIP events around 20 calls; the legs of a group alternate in one process, medians
and min .. max over 5 rounds.  All calls go through the probe build (the product entries in it are the same code).

usage: python tools/robot_box_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, CALLS, CAP = 5, 20, 4096


def scene(H, W, kind):
    """(gt, pred) uint8 [2,H,W], object 1 on frame 1: a disc of radius 100 around the middle; ``thick``: nothing of it is predicted,
    ``thin``: the prediction is the disc moved by 2 pixels in x and y, ``whole``: thick, plus the first and the last pixel of the frame."""
    import numpy as np
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((2, H, W), np.uint8)
    gt[1][(yy - H // 2) ** 2 + (xx - W // 2 + 7) ** 2 <= 100 * 100] = 1
    pred = np.roll(gt, (2, 2), (1, 2)) if kind == "thin" else np.zeros_like(gt)
    if kind == "whole":
        gt[1, 0, 0] = gt[1, H - 1, W - 1] = 1
    return gt, pred


class Leg:
    """One entry on one scene with its own output buffers; ``budget`` None: the product entry ``name``, else the probe with that budget."""

    def __init__(self, L, torch, dev, name, gt, pred, budget=None):
        self.L, self.torch, self.dev, self.name, self.budget = L, torch, dev, name, budget
        self.gt, self.pred = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        self.n, self.H, self.W = gt.shape
        self.buf = torch.zeros(2 + CAP, dtype=torch.int32, device=dev)
        import numpy as np
        self.units = np.ascontiguousarray(np.array([[1, 1]], np.int32))
        need = 2 * self.H * ((self.W + 31) // 32) * 4
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def __call__(self):
        L, lib = self.L, self.L.lib()
        args = [L.dptr(self.gt), L.dptr(self.pred), self.n, self.H, self.W, self.units.ctypes.data, 1, CAP, L.torch_ptr(self.buf, 2),
                L.dptr(self.buf), L.torch_ptr(self.buf, 1), None]
        if self.name == "old":
            rc = lib.ivosw_robot_skeleton(*args, L.stream_ptr(self.dev))
        elif self.budget is None:
            rc = lib.ivosw_robot_skeleton_box(*args, L.dptr(self.ws), self.ws.numel(), L.stream_ptr(self.dev))
        else:
            rc = lib.ivosw_robot_box_probe(*args, L.dptr(self.ws), self.ws.numel(), self.budget, L.stream_ptr(self.dev))
        L.check(rc, self.name)

    def result(self):
        h = self.buf.cpu().numpy()
        return int(h[0]), int(h[1]), h[2:2 + min(int(h[0]), CAP)].tobytes()

    def events(self):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            self()
        e1.record()
        torch.cuda.synchronize(self.dev)
        return e0.elapsed_time(e1) * 1e3 / CALLS              # us per call


def _fmt(v):
    return f"{statistics.median(v):9.1f} us  ({min(v):.1f} .. {max(v):.1f})"


def group(title, legs):
    """The legs alternate; their results must be the same bytes."""
    for leg in legs.values():
        for _ in range(3):
            leg()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            out[k].append(leg.events())
    res = {k: leg.result() for k, leg in legs.items()}
    first = next(iter(res.values()))
    assert all(r == first for r in res.values()), f"{title}: the legs disagree"
    print(f"{title}: {first[0]} skeleton pixels, {first[1]} iterations")
    base = None
    for k, v in out.items():
        med = statistics.median(v)
        base = med if base is None else base
        print(f"    {k:34s} {_fmt(v)}" + ("" if med == base else f"   {med / base:.2f} x the first"))
    return {k: statistics.median(v) for k, v in out.items()}


def main():
    import torch
    from ivos_w_amd import _lib as L
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    L.use_probe_lib()
    dev = torch.device("cuda:0")
    print(f"robot box probe: one unit per call, HIP events over {CALLS} calls, {ROUNDS} rounds alternating, medians (min .. max)")
    for kind in ("thick", "thin"):
        gt, pred = scene(480, 854, kind)
        group(f"480 x 854, {kind}", {"ivosw_robot_skeleton (full frame, LDS)": Leg(L, torch, dev, "old", gt, pred),
                                     "ivosw_robot_skeleton_box (LDS window)": Leg(L, torch, dev, "box", gt, pred)})
    for H, W in ((720, 1280), (1080, 1920)):
        for kind in ("thick", "thin"):
            gt, pred = scene(H, W, kind)
            group(f"{H} x {W}, {kind}", {"ivosw_robot_skeleton_box (LDS window)": Leg(L, torch, dev, "box", gt, pred)})
    gt, pred = scene(720, 1280, "whole")
    group("720 x 1280, whole-frame box", {"ivosw_robot_skeleton_box (global planes)": Leg(L, torch, dev, "box", gt, pred)})
    gt, pred = scene(720, 1280, "thick")
    group("720 x 1280, thick, the two plane homes", {"LDS window": Leg(L, torch, dev, "box", gt, pred),
                                                    "global planes (probe, 256 B of LDS)": Leg(L, torch, dev, "probe", gt, pred, budget=256)})


if __name__ == "__main__":
    main()
