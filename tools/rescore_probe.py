"""What the incremental assessment pass (rescore=changed: AssessNet.forward_videos_incremental) costs and gains against the full pass
(AssessNet.forward_videos), in ONE process on the GPU, at 480p in bf16: one 100-frame x 3-object video (300 units) and three of them.

  baseline      forward_videos(videos) + the copy of the score tables to the host - the full pass, code the incremental path does not
                touch;
  incremental   forward_videos_incremental(videos, caches) + the same copy, with 0, 1 unit, 10 %, 30 % and 100 % of the units dirty: before
                every timed call (outside the clock) one bit of one element of each chosen plane is flipped IN PLACE and the device is
                synchronised, so the call finds exactly those units changed;
  delta alone   ivosw_mask_delta_videos + the 4-byte copy of n_dirty, with nothing dirty (two plane reads per unit, no store) and with
                everything dirty (two reads and one store): us per call and GB/s against the HBM figures of the microarchitecture guide
                (8.0 TB/s peak, 6.3 TB/s measured with a float4 copy).

Every chain ends in a device-to-host copy, which synchronises; a reading is the host clock summed over REPS such chains after WARM warm-up
chains, the ways ALTERNATING over ROUNDS rounds.  The report gives the median, min .. max and the run-to-run spread (max - min) of each
way, the break-even dirty share (where the line through the two bracketing incremental medians meets the baseline median) and the
overhead at 100 %.  The incremental tables are compared bit for bit with the full pass at every share first.

usage: python tools/rescore_probe.py [--out FILE]        (the report goes to stdout, and to FILE: profiles/rescore_probe.txt)"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, T, O, ROUNDS, WARM, REPS = 480, 854, 100, 3, 5, 3, 10
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12                                      # bytes/s: spec peak, measured float4 copy (microarchitecture guide)


def _video(dev, n, n_obj, seed):
    """Random frames and soft blob masks (one blob per object and frame, drifting over the video), all on the device."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    frames = torch.rand(n, 3, H, W, generator=g, device=dev)
    yy = torch.arange(H, dtype=torch.float32, device=dev).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, 1, W)
    t = torch.arange(n, dtype=torch.float32, device=dev).view(n, 1, 1, 1) / max(n - 1, 1)
    o = torch.arange(n_obj + 1, dtype=torch.float32, device=dev).view(1, n_obj + 1, 1, 1)
    cy, cx, r = H * (0.3 + 0.3 * t + 0.05 * o), W * (0.2 + 0.5 * t + 0.07 * o), 40.0 + 25.0 * o + 30.0 * t
    all_P = torch.sigmoid((r - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) / 3.0).contiguous()
    return frames, all_P, n_obj


def _stats(say, name, v):
    say(f"  {name}  median {statistics.median(v):9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}   spread {max(v) - min(v):7.1f} us")
    return statistics.median(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ivos_w_amd import _lib as L
    from ivos_w_amd import synth
    from ivos_w_amd.models.assessment import AssessNet, ScoreCache
    dev = torch.device("cuda:0")
    lib = L.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# rescore_probe: one process; host clock around chains that end in a device-to-host copy; {WARM} warm-up chains, {REPS} timed "
        f"chains per reading, {ROUNDS} alternating rounds; {H} x {W}, bf16, videos of {T} frames x {O} objects")
    say(f"# device: {torch.cuda.get_device_name(dev)}")
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net = net.to(dev).eval()
    plane_bytes = 4 * H * W

    for n_videos in (1, 3):
        vids = [_video(dev, T, O, 100 * n_videos + k) for k in range(n_videos)]
        units = n_videos * T * O
        bits = [v[1].view(torch.int32) for v in vids]                      # the masks' own storage: pokes land where a ProbStore write would
        caches = [ScoreCache() for _ in vids]
        rs = np.random.RandomState(5)

        def poke(m):
            """Flip one bit in each of m distinct units' planes, in place; returns when the device has done it."""
            if m:
                pick = rs.choice(units, size=m, replace=False)
                for k in range(n_videos):
                    lu = pick[(pick >= k * T * O) & (pick < (k + 1) * T * O)] - k * T * O
                    if len(lu):
                        fr = torch.as_tensor(lu % T, device=dev)
                        ob = torch.as_tensor(1 + lu // T, device=dev)
                        bits[k][fr, ob, 0, 0] = bits[k][fr, ob, 0, 0] ^ 1
            torch.cuda.synchronize(dev)

        def full():
            return torch.cat([s.reshape(-1) for s in net.forward_videos(vids)]).cpu()

        def incremental():
            return torch.cat([s.reshape(-1) for s in net.forward_videos_incremental(vids, caches)]).cpu()

        def clocked(fn, m):
            total = 0.0
            for _ in range(REPS):
                poke(m)
                t0 = time.perf_counter()
                fn()                                                       # (ends in the copy to the host: synchronised)
                total += time.perf_counter() - t0
            return total / REPS * 1e6

        say(f"\n[{n_videos} video(s), {units} units: us per pass]")
        incremental()                                                      # cold: fills the caches
        shares = [("0", 0), ("1 unit", 1), ("10 %", units // 10), ("30 %", 3 * units // 10), ("100 %", units)]
        for _, m in shares:                                                # results first: bit-identical tables at every share
            poke(m)
            got, want = incremental(), full()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"incremental differs from the full pass at {m} dirty units"
            assert sum(c.rescored for c in caches) == m, (m, [c.rescored for c in caches])
        say(f" tables bit-identical to forward_videos at {', '.join(str(m) for _, m in shares)} dirty units; rescored counts as poked")
        for _ in range(WARM):
            poke(0)
            full()
            poke(units)
            incremental()
        res = {"all": []}
        res.update({name: [] for name, _ in shares})
        for _ in range(ROUNDS):
            res["all"].append(clocked(full, 0))
            for name, m in shares:
                res[name].append(clocked(incremental, m))
        base, base_spread = _stats(say, "baseline    forward_videos        ", res["all"])
        med = []
        for name, m in shares:
            md, _ = _stats(say, f"incremental {name:>7} dirty ({m:4d})", res[name])
            med.append((m / units, md))
        over = med[-1][1] - base
        say(f"  overhead at 100 % dirty: {over:+.1f} us ({100 * over / base:+.1f} % of the baseline; baseline spread {base_spread:.1f} us)")
        even = None
        for (s0, t0), (s1, t1) in zip(med, med[1:]):
            if t0 <= base < t1:
                even = s0 + (s1 - s0) * (base - t0) / (t1 - t0)
        if med[0][1] > base:
            say("  break-even: none - the incremental pass is slower than the baseline with nothing dirty")
        elif even is None:
            say("  break-even: none below 100 % - the incremental pass is not slower than the baseline at any measured share")
        else:
            say(f"  break-even dirty share: {100 * even:.0f} % (linear between the bracketing medians)")

        # the delta pass alone
        arr_keep = []
        descs = [net._video_entry(k, v, arr_keep)[0] for k, v in enumerate(vids)]
        arr = (L.Video * n_videos)(*descs)
        ptrs = (ctypes.c_void_p * n_videos)(*[c.planes.data_ptr() for c in caches])
        meta = torch.empty(2 * units + 1, dtype=torch.int32, device=dev)
        flags, ids, nd = meta[:units], meta[units:2 * units], meta[2 * units:]
        cold = L.int_array([0] * n_videos)

        def delta():
            L.check(lib.ivosw_mask_delta_videos(arr, n_videos, ptrs, cold, L.dptr(flags), L.dptr(ids), L.dptr(nd), L.stream_ptr(dev)), "mask_delta_videos")
            return int(nd.item())

        def every_plane():                                                 # every unit dirty: one bit of every plane, outside the clock
            for k in range(n_videos):
                bits[k][:, 1:, 0, 0] ^= 1
            torch.cuda.synchronize(dev)
        say(f" delta pass alone (ivosw_mask_delta_videos + the 4-byte copy), us per call; {2 * plane_bytes * units / 1e6:.0f} MB read per call")
        dres = {"clean": [], "dirty": []}
        for _ in range(WARM):
            assert delta() == 0
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                delta()
            dres["clean"].append((time.perf_counter() - t0) / REPS * 1e6)
            tot = 0.0
            for _ in range(REPS):
                every_plane()
                t0 = time.perf_counter()
                n = delta()
                tot += time.perf_counter() - t0
                assert n == units
            dres["dirty"].append(tot / REPS * 1e6)
        for key, label, nbytes in (("clean", "nothing dirty (2 reads)          ", 2 * plane_bytes * units),
                                   ("dirty", "all dirty, one vector per plane  ", 2 * plane_bytes * units)):
            md, _ = _stats(say, label, dres[key])
            rate = nbytes / (md * 1e-6)
            say(f"      {rate / 1e9:7.0f} GB/s = {100 * rate / HBM_PEAK:.0f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:.0f} % of the 6.3 TB/s copy rate; "
                f"{md / units:.2f} us per unit against {base / units:.2f} us per unit of the full pass")
        del vids, bits, caches, meta, arr_keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
