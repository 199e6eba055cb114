"""The ragged recommendation chain - quality -> state -> Brain -> masked top-k -> one D2H copy - ending in the spread ranking
(ivosw_brain_topk_spread_ragged, agent.candidate_gap = 5) against the same chain ending in ivosw_brain_topk_ragged (gap = 1, today's
calls), in ONE process (GPU only).

For K x T in {1 x 30, 32 x 30, 8 x 100, 32 x 100} sessions of T frames with 1 to 3 objects (cycling) and k in {4, 16} candidates, scores
and counts on the device, both ways run ivosw_quality_state_ragged + Brain.forward_ragged (three launches) + their last launch with
skip_annotated, and end in the device-to-host copy of [quality (R) | K k indices], which synchronises:
  (g1)  Agent.topk_ragged at gap = 1: ivosw_brain_topk_ragged          - the baseline, timed in the same run;
  (g5)  Agent.topk_ragged at gap = 5: ivosw_brain_topk_spread_ragged, with a forced first candidate for every third session.
Five launches and one copy either way.  A reading is the host clock around REPS such chains (the method of tools/topk_probe.py), after WARM
warm-up chains, the two ways ALTERNATING over ROUNDS rounds.  The report gives each way's median, min .. max and run-to-run spread
(max - min), and the difference (g5) - (g1) against the larger of the two spreads.  Before timing, the spread entry at gap = 1 without
forced candidates is compared with the plain entry, and the gap = 5 ranking is checked to be 5 apart with candidate 0 unchanged where
nothing is forced.

usage: python tools/spread_probe.py [--out FILE]        (the report goes to stdout, and to FILE: profiles/spread_probe.txt)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, WARM, REPS = 5, 10, 50
CASES = [(1, 30), (32, 30), (8, 100), (32, 100)]
KS = (4, 16)
GAP = 5


class AD(dict):
    __getattr__ = dict.__getitem__


def _clocked(fn, reps, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()                                                             # (every fn ends in a device-to-host copy: synchronised)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / reps * 1e6                       # us per chain


def _alternate(legs, dev):
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            out[k].append(_clocked(fn, REPS, dev))
    return out


def _legs(dev, agent, K, T, k):
    import torch
    from ivos_w_amd import _lib as L
    lib = L.lib()
    n_obj = [1 + s % 3 for s in range(K)]
    g = torch.Generator(device=dev).manual_seed(1000 * K + T)
    scores = torch.rand(sum(n_obj) * T, generator=g, device=dev)
    cnt = torch.randint(0, 3, (K * T,), generator=g, device=dev).float()
    lengths, R = [T] * K, K * T
    forced = [(7 * s) % T if s % 3 == 0 else -1 for s in range(K)]
    kept = {}

    def chain(key, gap, first):
        out = torch.zeros(R + K * k, dtype=torch.float64, device=dev)
        state = torch.empty(R, 2, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_quality_state_ragged(L.dptr(scores), L.int_array(n_obj), L.int_array(lengths), K, L.dptr(cnt), L.dptr(out),
                                               L.dptr(state), L.stream_ptr(dev)), "quality_state_ragged")
        q, _ = agent.policy_net.forward_ragged(state, lengths)
        agent.topk_ragged(q, state, lengths, k, True, out=out[R:].view(torch.int64), gap=gap, first=first)    # gap 1, no first: the plain entry
        kept[key] = out.cpu()

    def index(key):
        return kept[key][R:].view(torch.int64).view(K, k)
    chain("g1", 1, None)
    chain("same", 1, [-1] * K)                                           # a `first` at gap = 1: the spread entry itself
    assert torch.equal(index("g1"), index("same")), "the spread entry at gap = 1 differs from the plain entry"
    chain("g5", GAP, forced)
    for s, row in enumerate(index("g5").tolist()):
        got = [t for t in row if t >= 0]
        assert got and all(abs(a - b) >= GAP for i, a in enumerate(got) for b in got[:i]), (s, row)
        assert got[0] == (forced[s] if forced[s] >= 0 else int(index("g1")[s, 0])), (s, row)
    return {"g1": lambda: chain("g1", 1, None), "g5": lambda: chain("g5", GAP, forced)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from ivos_w_amd import synth
    from ivos_w_amd.models.agent import Agent
    dev = torch.device("cuda:0")
    cfg = AD(phase="eval", data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                           update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# spread_probe: one process; host clock around chains that end in the D2H copy; {WARM} warm-up chains, {REPS} timed chains per "
        f"reading, {ROUNDS} alternating rounds")
    say(f"# device: {torch.cuda.get_device_name(dev)}")
    say(f"\n[quality -> state -> ragged Brain -> masked top-k at gap 1 | gap {GAP} -> D2H, us per chain over K sessions of T frames]")
    names = {"g1": "(g1) topk_ragged, gap = 1        ", "g5": f"(g5) topk_spread_ragged, gap = {GAP} "}
    for K, T in CASES:
        for k in KS:
            say(f" K = {K}, T = {T}, k = {k}, objects 1..3")
            res = _alternate(_legs(dev, agent, K, T, k), dev)
            med = {w: statistics.median(v) for w, v in res.items()}
            spread = {w: max(v) - min(v) for w, v in res.items()}
            for w in res:
                say(f"  {names[w]}  median {med[w]:8.1f} us   min {min(res[w]):8.1f}   max {max(res[w]):8.1f}   spread {spread[w]:6.1f} us")
            diff, worst = med["g5"] - med["g1"], max(spread.values())
            verdict = "inside the spread" if abs(diff) <= worst else ("slower by more than the spread" if diff > 0 else "faster by more than the spread")
            say(f"  (g5) - (g1) = {diff:+6.1f} us ({med['g5'] / med['g1']:.3f} x); larger run-to-run spread {worst:.1f} us: {verdict}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
