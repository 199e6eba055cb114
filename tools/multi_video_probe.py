"""Several videos in one assessment pass against one pass per video, 480p, bf16 (GPU only), in ONE process.

For K = 1, 2, 3 videos of 100 frames x 1 object and for 2 videos of 70 frames x 2 objects:
  (a) sequential   K calls of AssessNet.forward_objects, one per video - what a caller with K sessions had to do before;
  (b) one pass     one call of AssessNet.forward_videos over the K videos.
Warm-up and repeats as in bench.py's eval_sizes leg (6 calls, then 30 timed between two HIP events), the two ways ALTERNATING over
ROUNDS rounds; the report gives units/s of both (median, min .. max over the rounds), the run-to-run spread of (a), and whether (b) sits
inside it.  At K = 1 the two ways run the same tower on the same tiles: (b) must sit inside (a)'s spread.
Then the front end alone (mask -> box, ROI sampler; HIP events around 50 launches): the multi-video kernels over K videos against the
single-video kernels run per video, as time per unit, with the table lookup's cost put against the single-video sampler.

usage: python tools/multi_video_probe.py [--out FILE]        (the report goes to stdout, and to FILE: profiles/multi_video_probe.txt)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, ROUNDS, WARM, REPS, FRONT_REPS = 480, 854, 5, 6, 30, 50
CASES = [(1, 100, 1), (2, 100, 1), (3, 100, 1), (2, 70, 2)]          # (videos, frames, objects)


def _video(dev, n, O, seed):
    """Random frames and soft blob masks (one blob per object and frame, drifting over the video), all on the device."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    frames = torch.rand(n, 3, H, W, generator=g, device=dev)
    yy = torch.arange(H, dtype=torch.float32, device=dev).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, 1, W)
    t = torch.arange(n, dtype=torch.float32, device=dev).view(n, 1, 1, 1) / max(n - 1, 1)
    o = torch.arange(O + 1, dtype=torch.float32, device=dev).view(1, O + 1, 1, 1)
    cy, cx, r = H * (0.3 + 0.3 * t + 0.05 * o), W * (0.2 + 0.5 * t + 0.07 * o), 40.0 + 25.0 * o + 30.0 * t
    all_P = torch.sigmoid((r - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) / 3.0).contiguous()
    return frames, all_P, O


def _timed(fn, reps, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps                                  # ms per call


def _alternate(legs, reps, dev):
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            out[k].append(_timed(fn, reps, dev))
    return out


def _front_legs(dev, vids):
    """The front end alone over the units of `vids`: single-video kernels per video against the multi-video kernels in one launch."""
    import torch
    from ivos_w_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    units = sum(f.shape[0] * O for f, _, O in vids)
    yxhw = torch.empty(units, 4, device=dev)
    scratch = torch.empty(units * 4, dtype=torch.int32, device=dev)
    roi = torch.empty(units, 256, 256, 4, dtype=torch.bfloat16, device=dev)
    arr = (L.Video * len(vids))(*[L.Video(f.data_ptr(), P[:, 1:].data_ptr(), P.stride(0), P.stride(1), L.FRAMES_F32, f.shape[0], O, H, W)
                                  for f, P, O in vids])
    # the single-video entries take one mask plane per unit and one frame per unit (O = 1 in the cases timed here)
    singles, off = [], 0
    for f, P, O in vids:
        assert O == 1
        singles.append((f, P[:, 1].contiguous(), off, f.shape[0]))
        off += f.shape[0]

    def bbox_single():
        for f, m, o, n in singles:
            L.check(lib.ivosw_mask_bbox(L.dptr(m), n, H, W, L.dptr(yxhw[o:o + n]), L.dptr(scratch[4 * o:4 * (o + n)]), st))

    def bbox_multi():
        L.check(lib.ivosw_mask_bbox_videos(arr, len(vids), L.dptr(yxhw), L.dptr(scratch), st))

    def roi_single():
        for f, m, o, n in singles:
            L.check(lib.ivosw_roi_sample(L.dptr(f), L.dptr(m), L.dptr(yxhw[o:o + n]), n, H, W, L.BF16, L.dptr(roi[o:o + n]), st))

    def roi_multi():
        L.check(lib.ivosw_roi_sample_videos(arr, len(vids), L.dptr(yxhw), L.BF16, L.dptr(roi), st))
    bbox_multi()
    return {"bbox single": bbox_single, "bbox multi": bbox_multi, "roi single": roi_single, "roi multi": roi_multi}, units


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ivos_w_amd import synth
    from ivos_w_amd.models.assessment import AssessNet
    dev = torch.device("cuda:0")
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net = net.to(dev).eval()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# multi_video_probe: {H} x {W}, bf16, one process; {WARM} warm-up calls, {REPS} timed calls per reading, {ROUNDS} alternating rounds")
    say(f"# device: {torch.cuda.get_device_name(dev)}")
    pool = {}
    for K, n, O in CASES:
        for k in range(K):
            if (k, n, O) not in pool:
                pool[(k, n, O)] = _video(dev, n, O, 100 * k + n + O)
        vids = [pool[(k, n, O)] for k in range(K)]
        units = K * n * O
        want = [net.forward_objects(*v) for v in vids]
        got = net.forward_videos(vids)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), "forward_videos differs from forward_objects"
        res = _alternate({"a": lambda: [net.forward_objects(*v) for v in vids], "b": lambda: net.forward_videos(vids)}, REPS, dev)
        ups = {k: [units / ms * 1e3 for ms in v] for k, v in res.items()}
        ma, mb = statistics.median(ups["a"]), statistics.median(ups["b"])
        spread = max(ups["a"]) - min(ups["a"])
        verdict = "above (a)'s spread" if mb - ma > spread else ("BELOW (a)'s spread" if ma - mb > spread else "inside (a)'s spread")
        say(f"\n[{K} x {n} frames x {O} objects = {units} units]  scores bit-identical")
        for k, name in (("a", "(a) sequential forward_objects"), ("b", "(b) one forward_videos      ")):
            say(f"  {name}  median {statistics.median(ups[k]) / 1e3:7.2f} k units/s   min {min(ups[k]) / 1e3:7.2f}   max {max(ups[k]) / 1e3:7.2f}"
                f"   ({statistics.median(res[k]):7.3f} ms per {units} units)")
        say(f"  (b) - (a) = {(mb - ma) / 1e3:+.2f} k units/s ({100 * (mb - ma) / ma:+.1f} %); run-to-run spread of (a) {spread / 1e3:.2f} k units/s "
            f"({100 * spread / ma:.1f} %): (b) is {verdict}")
    say("\n[front end alone, us per unit: the single-video kernels run per video against the multi-video kernels in one launch]")
    for K in (1, 3):
        vids = [pool[(k, 100, 1)] for k in range(K)]
        legs, units = _front_legs(dev, vids)
        res = _alternate(legs, FRONT_REPS, dev)
        for name in legs:
            us = [ms * 1e3 / units for ms in res[name]]
            say(f"  K = {K}  {name:<12} median {statistics.median(us):7.4f} us/unit   min {min(us):7.4f}   max {max(us):7.4f}"
                f"   ({statistics.median(res[name]) * 1e3:8.2f} us per {units} units)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
