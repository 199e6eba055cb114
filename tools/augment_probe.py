"""What the fused augmentation warp costs on the device, against the host sequence it replaces.

Conditions: 480 x 854, 32 samples (the reference's train_batch_size) of one 8-frame, 2-object video resident on the device, output
480 x 854, the reference's train transform (Resize, RandomAffine, AdditiveNoise, RandomContrast, RandomHorizontalFlip); frame kinds
fp32 and RGBX8; with 12 candidates per sample and with none (the pipeline without RandomAffine).
  (a) batch    device: transforms_assess.Compose on a DeviceSamples (the draws, ONE ivosw_qa_augment call), then a synchronise
               host:   the numpy restatement of the same rule (tests/augment_ref.py) on host copies of the sources plus the upload of
                       the float sample (img float32 [N,3,H,W] and prob, as the reference's ToTensor + pinned upload).  cv2 and imgaug
                       are not part of this project's environment and could not be timed; the restatement stands in for them.
                       The two ways are checked for equal bits while they are timed.
  (b) warp     the warp launches alone: device events around REPS C calls with a sample table built beforehand (transforms_assess.launch:
               nothing but the ctypes call runs between the events), as bytes moved over time: per output pixel 18 B written (img, prob,
               label, mask) and 14 B (fp32 frames) or 6 B (RGBX8) read.  Events see max(host, device), so the host time of one C call
               (clock around the call, no synchronise) stands beside every event figure: it must be the smaller one.
  (c) select   the selection launches: the C call with 12 candidates per sample against the C call that warps THE SAME maps without
               candidates (n_cand = 0, post = the map the device chose, so both warps gather alike), both with prebuilt tables
Host clock around chains that end in a synchronise for (a); the ways alternate inside one process; medians of ROUNDS rounds with
min .. max.

    python tools/augment_probe.py [--out profiles/augment_probe.txt] [--rounds 5]
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ivos_w_amd  # noqa: E402,F401
from ivos_w_amd.datasets import transforms_assess as T  # noqa: E402
from ivos_w_amd.models.assessment import PackedFrames  # noqa: E402
from tests import augment_ref as R  # noqa: E402

H, W, NF, O, N = 480, 854, 8, 2, 32


def make_video(u8, seed):
    g = np.random.RandomState(seed)
    coarse = g.randint(0, O + 1, (NF, 12, 14)).astype(np.uint8)
    gt = np.ascontiguousarray(np.repeat(np.repeat(coarse, 40, 1), 61, 2)[:, :H, :W])
    planes = np.where(gt[None] == np.arange(1, O + 1)[:, None, None, None], 230, 20).astype(np.uint8) + g.randint(0, 16, (O, NF, H, W)).astype(np.uint8)
    frames = g.randint(0, 256, (NF, H, W, 4)).astype(np.uint8) if u8 else g.rand(NF, 3, H, W).astype(np.float32)
    return dict(frames=frames, gt=gt, planes=planes, obj_ids=list(range(1, O + 1)))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, r


def host_ms(fn, dev, reps=20):
    """Host time of one call of fn, the device left to run behind (synchronised before and after the batch only)."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize(dev)
    return t


def event_ms(fn, dev, reps=20):
    fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def fmt(xs):
    return f"{np.median(xs):9.3f}  ({min(xs):.3f} .. {max(xs):.3f})"


def pipeline(with_affine, size=(W, H)):
    steps = [T.Resize(size=size)] + ([T.RandomAffine()] if with_affine else []) + [T.AdditiveNoise(), T.RandomContrast(), T.RandomHorizontalFlip()]
    return T.Compose(steps + [T.ToTensor()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    units = [(0, k % NF, k % O) for k in range(N)]
    lines = [f"augment_probe: {H} x {W} -> {H} x {W}, {N} samples, medians of {args.rounds} alternating rounds (min .. max), ms",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for u8 in (False, True):
        vid = make_video(u8, 3 + u8)
        fr = torch.from_numpy(vid["frames"]).to(dev)
        ds = T.DeviceSamples([(PackedFrames(fr) if u8 else fr, torch.from_numpy(vid["gt"]).to(dev), torch.from_numpy(vid["planes"]).to(dev))], units)
        kind = "RGBX8" if u8 else "fp32"
        lines.append(f"--- frames {kind}")
        warp_ms = None
        for with_affine in (True, False):
            pipe = pipeline(with_affine)

            def device_way(seed):
                random.seed(seed)
                np.random.seed(seed)
                return pipe(ds)

            def host_way(seed):
                random.seed(seed)
                np.random.seed(seed)
                rows, (Wo, Ho) = pipe.draw(ds.sizes())
                out = R.augment([vid], [dict(v=v, f=f, o=o, **r) for (v, f, o), r in zip(units, rows)], Ho, Wo)
                up = [torch.from_numpy(out["img"]).pin_memory().to(dev, non_blocking=True), torch.from_numpy(out["prob"]).pin_memory().to(dev, non_blocking=True)]
                return out, up
            device_way(0)
            td, th = [], []
            for r in range(args.rounds):
                for way in (("device", "host") if r % 2 == 0 else ("host", "device")):
                    if way == "device":
                        ms, got = timed(lambda: device_way(100 + r), dev)
                        td.append(ms)
                        got = {k: t.cpu().numpy() for k, t in got.items()}
                    else:
                        ms, (want, _) = timed(lambda: host_way(100 + r), dev)
                        th.append(ms)
                for k in want:
                    assert got[k].tobytes() == want[k].tobytes(), f"device and host differ in {k}"
            name = "12 candidates" if with_affine else "no candidate "
            lines.append(f"(a) batch, {name}  device {fmt(td)}    host (numpy restatement + upload) {fmt(th)}    x{np.median(th) / np.median(td):.1f}"
                         f"    results: equal bits")
        # the C call alone, tables built beforehand: (b) the no-candidate pipeline, (c) 12 candidates against the same maps without
        def prebuilt(rows, Ho, Wo):
            table, any_cand = T.sample_table(ds, rows)
            out, ws = T.empty_outputs(N, Ho, Wo, dev), T.workspace(N, dev)
            return (lambda: T.launch(ds, table, any_cand, Ho, Wo, out, ws)), out
        random.seed(1)
        np.random.seed(1)
        rows, (Wo, Ho) = pipeline(False).draw(ds.sizes())
        call, _ = prebuilt(rows, Ho, Wo)
        warp_ms = [event_ms(call, dev) for _ in range(args.rounds)]
        warp_host = [host_ms(call, dev) for _ in range(args.rounds)]
        bpp = 18 + (6 if u8 else 14)
        tbs = [bpp * N * H * W / (ms * 1e-3) / 1e12 for ms in warp_ms]
        lines.append(f"(b) warp launches alone  {fmt(warp_ms)} ms = {np.median(tbs):.2f} TB/s ({min(tbs):.2f} .. {max(tbs):.2f}) over {bpp} B / pixel"
                     f"  [float4 copy: 6.3 TB/s]    host time of the call {fmt(warp_host)}")
        random.seed(1)
        np.random.seed(1)
        rows, (Wo, Ho) = pipeline(True).draw(ds.sizes())
        with_sel, out = prebuilt(rows, Ho, Wo)
        with_sel()
        chosen = out["chosen"].cpu().numpy()
        same_maps = []
        for r, c in zip(rows, chosen):
            post = np.array([r["post"][:3], r["post"][3:], [0., 0., 1.]])
            full = post if c == len(r["cands"]) else np.array([r["cands"][c][:3], r["cands"][c][3:], [0., 0., 1.]]) @ post
            same_maps.append(dict(post=T._six(full), noise=r["noise"], contrast=r["contrast"]))
        without_sel, _ = prebuilt(same_maps, Ho, Wo)
        ta, tb = [], []
        for r in range(args.rounds):
            for way in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tb if way else ta).append(event_ms(without_sel if way else with_sel, dev))
        sel_host = [host_ms(with_sel, dev) for _ in range(args.rounds)]
        lines += [f"(c) call, 12 candidates  {fmt(ta)}    the same maps, no candidates {fmt(tb)}    selection launches = the difference "
                  f"{np.median(ta) - np.median(tb):.3f} ms    host time of the call {fmt(sel_host)}    chosen: {np.bincount(chosen, minlength=13).tolist()}", ""]
        del ds, fr
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
