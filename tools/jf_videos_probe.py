"""What the host detour of J / F costs an oracle interaction, and what the one-pass device chain costs instead.

Conditions: 480p (480 x 854) label maps resident on the device, 100 and 30 frames, 1 and 3 objects, K = 1, 2, 8, 32 open sessions.
  metric  per-video: misc.sequence_metric per session (two launches, the counts copied back, the ratios in Python)
          one pass:  misc.sequence_metric_videos over all sessions (ivosw_jf_counts_videos + ivosw_jf_reduce_ragged, one copy)
  tail    per-video: sequence_metric + recommend_frame (setting oracle, method ours) per session
          one pass:  utils_agent.oracle_recommend over all sessions (the same pass with the Brain's state filled on the device, the
                     ragged Brain chain, one copy of [quality | indices])
Host clock around chains that end in their synchronising copy; the two ways alternate inside one process; medians of ROUNDS rounds with
min .. max.  The baseline is the per-video path of the same run.  Results are checked for bit equality while they are timed.

    python tools/jf_videos_probe.py [--out profiles/jf_videos_probe.txt] [--rounds 5]
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
from ivos_w_amd import synth  # noqa: E402
from ivos_w_amd.models.agent import Agent  # noqa: E402
from ivos_w_amd.utils import misc, utils_agent  # noqa: E402

H, W = 480, 854
METRIC = "J_AND_F"


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_sessions(dev, K, n, O, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for _ in range(K):
        coarse = torch.randint(0, O + 1, (n, 12, 14), generator=g, dtype=torch.uint8).to(dev)
        gt = coarse.repeat_interleave(40, 1).repeat_interleave(61, 2)[:, :H, :W].contiguous()
        pred = torch.roll(gt, (3, -5), (1, 2)).contiguous()
        out.append(dict(gt_masks=gt, pred_masks=pred, n_objects=O, annotated_frames_list=[0, n // 2], prev_frames=[0, n // 2]))
    return out


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    return f"{np.median(ms):8.2f} ({min(ms):7.2f} .. {max(ms):7.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jf_videos_probe.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                          update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    cy = AD(setting="oracle", method="ours", davis_interactive=AD(metric=METRIC))
    lines = [f"jf_videos_probe: {torch.cuda.get_device_name(dev)}, {H} x {W} uint8 label maps on the device, metric {METRIC}, ms per call "
             f"(all K sessions), median of {args.rounds} rounds (min .. max), the two ways alternating",
             f"{'frames':>6} {'obj':>3} {'K':>3} | {'metric per-video':>28} {'metric one pass':>28} {'x':>5} | {'tail per-video':>28} "
             f"{'tail one pass':>28} {'x':>5}"]
    import builtins
    real_print = builtins.print

    def per_video_metric(sessions):
        return [misc.sequence_metric(METRIC, s["gt_masks"], s["pred_masks"], s["n_objects"]) for s in sessions]

    def one_pass_metric(sessions):
        return misc.sequence_metric_videos(METRIC, [(s["gt_masks"], s["pred_masks"], s["n_objects"]) for s in sessions])

    def per_video_tail(sessions):
        ms, picks = [], []
        for s in sessions:
            m = misc.sequence_metric(METRIC, s["gt_masks"], s["pred_masks"], s["n_objects"])
            picks.append(int(utils_agent.recommend_frame(cy, None, agent, dev, n_frame=len(m), n_objects=s["n_objects"], all_F=None, all_P=None,
                                                         new_masks_quality=m, prev_frames=s["prev_frames"],
                                                         annotated_frames_list=list(s["annotated_frames_list"]), mask_quality=None,
                                                         first_frame=0, max_nb_interactions=8)))
            ms.append(m)
        return ms, picks

    def one_pass_tail(sessions):
        ms, picks = utils_agent.oracle_recommend(cy, agent, dev, sessions)
        return ms, [int(p) for p in picks]

    builtins.print = lambda *a, **k: None                    # Agent.action logs a line per call: keep the terminal out of the timings
    try:
        for n in (100, 30):
            for O in (1, 3):
                for K in (1, 2, 8, 32):
                    sessions = make_sessions(dev, K, n, O, seed=1000 * n + 10 * O + K)
                    random.seed(0)
                    for fn in (per_video_metric, one_pass_metric, per_video_tail, one_pass_tail):      # warm-up: allocator, workspaces
                        fn(sessions)
                    t = {k: [] for k in ("pm", "om", "pt", "ot")}
                    for _ in range(args.rounds):
                        a, ra = timed(lambda: per_video_metric(sessions), dev)
                        b, rb = timed(lambda: one_pass_metric(sessions), dev)
                        c, rc = timed(lambda: per_video_tail(sessions), dev)
                        d, rd = timed(lambda: one_pass_tail(sessions), dev)
                        assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(ra, rb))
                        assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(rc[0], rd[0])) and rc[1] == rd[1]
                        for key, v in zip(("pm", "om", "pt", "ot"), (a, b, c, d)):
                            t[key].append(v)
                    lines.append(f"{n:6d} {O:3d} {K:3d} | {stats(t['pm'])} {stats(t['om'])} {np.median(t['pm']) / np.median(t['om']):5.2f} | "
                                 f"{stats(t['pt'])} {stats(t['ot'])} {np.median(t['pt']) / np.median(t['ot']):5.2f}")
                    real_print(lines[-1], flush=True)
                    del sessions
                    torch.cuda.empty_cache()
    finally:
        builtins.print = real_print
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2]))
    print(f"written to {args.out}")


if __name__ == "__main__":
    main()
