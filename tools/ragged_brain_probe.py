"""The tail of utils_agent.recommend_frames - quality -> state -> Brain -> argmax -> one D2H copy - as K per-request chains against ONE
ragged chain, and whole recommend_frames calls both ways (GPU only), in ONE process.

Chain alone, for K in {2, 3, 8, 32} sessions of T in {30, 100} frames with 1 to 3 objects (cycling), scores and counts on the device:
  (a) per request   per session ivosw_quality_state + Agent.action(device_out=...) (fused encoder, N = 1 recurrence, fused decoder, argmax):
                    5 K launches - the loop recommend_frames ran before the ragged entries, reproduced from the single entries;
  (b) ragged        ivosw_quality_state_ragged + Agent.actions(device_out=...): 5 launches whatever K is.
Both end in the one device-to-host copy of [quality | indices], which synchronises; a reading is the host clock around REPS such chains
(launch overhead is what is being compared, so the host's time counts), after WARM warm-up chains, the two ways ALTERNATING over ROUNDS
rounds.  The report gives the median, min .. max over the rounds, the run-to-run spread of each way (max - min), and whether the
difference of the medians exceeds the larger spread.  The two ways' outputs are compared bit for bit first.

Whole calls: utils_agent.recommend_frames under wild/ours at 480p in bf16, K sessions of T frames, the videos resident on the device,
with RAGGED_MIN_REQUESTS at its committed value against RAGGED_MIN_REQUESTS = infinity (the per-request loop of the parent commit).

usage: python tools/ragged_brain_probe.py [--out FILE]        (the report goes to stdout, and to FILE: profiles/ragged_brain_probe.txt)"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, ROUNDS, WARM, REPS, CALL_REPS = 480, 854, 5, 10, 50, 8
CHAIN_CASES = [(K, T) for T in (30, 100) for K in (2, 3, 8, 32)]
CALL_CASES = [(2, 30), (3, 30), (8, 30), (32, 30), (2, 100), (8, 100)]


class AD(dict):
    __getattr__ = dict.__getitem__


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


def _clocked(fn, reps, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()                                                             # (every fn ends in a device-to-host copy: synchronised)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / reps * 1e6                       # us per call


def _alternate(legs, reps, dev, warm=WARM):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            out[k].append(_clocked(fn, reps, dev))
    return out


def _report(say, res, names):
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    for k in res:
        say(f"  {names[k]}  median {med[k]:9.1f} us   min {min(res[k]):9.1f}   max {max(res[k]):9.1f}   spread {spread[k]:7.1f} us")
    a, b = list(res)
    worst = max(spread.values())
    diff = med[a] - med[b]
    verdict = "faster by more than the spread" if diff > worst else ("SLOWER by more than the spread" if -diff > worst else "inside the spread")
    say(f"  (a) - (b) = {diff:+.1f} us ({med[a] / med[b]:.2f} x); larger run-to-run spread {worst:.1f} us: (b) is {verdict}")
    return diff, worst


def _chain_legs(dev, agent, K, T):
    import numpy as np
    import torch
    from ivos_w_amd import _lib as L
    lib = L.lib()
    n_obj = [1 + k % 3 for k in range(K)]
    g = torch.Generator(device=dev).manual_seed(1000 * K + T)
    scores = torch.rand(sum(n_obj) * T, generator=g, device=dev)
    cnt = torch.randint(0, 3, (K * T,), generator=g, device=dev).float()
    uoff = np.concatenate([[0], np.cumsum([o * T for o in n_obj])])
    lengths = [T] * K
    kept = {}

    def per_request():
        out = torch.zeros(K * (T + 1), dtype=torch.float64, device=dev)
        for k in range(K):
            o = k * (T + 1)
            state = torch.empty(T, 2, dtype=torch.float32, device=dev)
            L.check(lib.ivosw_quality_state(L.dptr(scores[int(uoff[k]):int(uoff[k + 1])]), n_obj[k], T, L.dptr(cnt[k * T:(k + 1) * T]),
                                            L.dptr(out[o:o + T]), L.dptr(state), L.stream_ptr(dev)), "quality_state")
            agent.action(state, verbose=False, device_out=out[o + T:o + T + 1].view(torch.int64))
        kept["a"] = out.cpu()

    def ragged():
        R = K * T
        out = torch.zeros(R + K, dtype=torch.float64, device=dev)
        state = torch.empty(R, 2, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_quality_state_ragged(L.dptr(scores), L.int_array(n_obj), L.int_array(lengths), K, L.dptr(cnt), L.dptr(out),
                                               L.dptr(state), L.stream_ptr(dev)), "quality_state_ragged")
        agent.actions([state[k * T:(k + 1) * T] for k in range(K)], verbose=False, device_out=out[R:].view(torch.int64))
        kept["b"] = out.cpu()
    per_request()
    ragged()
    a, b = kept["a"].view(torch.int64).view(K, T + 1), kept["b"].view(torch.int64)
    assert torch.equal(a[:, :T].reshape(-1), b[:K * T]) and torch.equal(a[:, T], b[K * T:]), "the ragged chain differs from the per-request chains"
    return {"a": per_request, "b": ragged}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ivos_w_amd import synth
    from ivos_w_amd.models.agent import Agent
    from ivos_w_amd.models.assessment import AssessNet
    from ivos_w_amd.utils import utils_agent
    dev = torch.device("cuda:0")
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# ragged_brain_probe: one process; host clock around calls that end in the D2H copy; {WARM} warm-up calls, {REPS} timed chains "
        f"({CALL_REPS} whole calls) per reading, {ROUNDS} alternating rounds")
    say(f"# device: {torch.cuda.get_device_name(dev)}")
    say("\n[chain alone: quality -> state -> Brain -> argmax -> D2H, us per chain over K sessions; outputs bit-identical]")
    wins = {}
    names = {"a": "(a) K per-request chains", "b": "(b) one ragged chain    "}
    for K, T in CHAIN_CASES:
        say(f" K = {K}, T = {T}, objects 1..3")
        diff, worst = _report(say, _alternate(_chain_legs(dev, agent, K, T), REPS, dev), names)
        wins[(K, T)] = (diff, worst)
    slower = sorted({K for (K, T), (d, w) in wins.items() if -d > w})
    say(f"\n K at which the ragged chain is slower than the per-request chains by more than the spread: {slower if slower else 'none'}")

    say(f"\n[whole recommend_frames calls, wild/ours, {H} x {W}, bf16, videos on the device, us per call]")
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net = net.to(dev).eval()
    cy = AD(setting="wild", method="ours")
    committed = utils_agent.RAGGED_MIN_REQUESTS
    names = {"a": "(a) per-request tail (parent)", "b": f"(b) ragged tail from K >= {committed}   "}
    for K, T in CALL_CASES:
        vids = [_video(dev, T, 1 + k, 10 * T + k) for k in range(3)]       # three videos (1, 2, 3 objects), shared by the K sessions in turn
        reqs = [dict(n_frame=T, n_objects=vids[k % 3][2], all_F=vids[k % 3][0], all_P=vids[k % 3][1], new_masks_quality=np.zeros(T),
                     prev_frames=[1], annotated_frames_list=[1, 1, 0], mask_quality=np.zeros(T), first_frame=1, max_nb_interactions=8)
                for k in range(K)]
        got = {}

        def call(threshold, key):
            utils_agent.RAGGED_MIN_REQUESTS = threshold
            try:
                with contextlib.redirect_stdout(io.StringIO()):              # (agent.action's log line, the same K lines both ways)
                    got[key] = [int(i) for i in utils_agent.recommend_frames(cy, net, agent, dev, reqs)]
            finally:
                utils_agent.RAGGED_MIN_REQUESTS = committed
        legs = {"a": lambda: call(1 << 30, "a"), "b": lambda: call(committed, "b")}
        legs["a"]()
        qa = [r["mask_quality"].copy() for r in reqs]
        legs["b"]()
        assert got["a"] == got["b"] and all(np.array_equal(x, r["mask_quality"]) for x, r in zip(qa, reqs)), "the two tails disagree"
        say(f" K = {K}, T = {T}: {sum(T * r['n_objects'] for r in reqs)} units, indices and quality identical")
        _report(say, _alternate(legs, CALL_REPS, dev, warm=3), names)
        del vids, reqs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
