"""The ragged recommendation chain - quality -> state -> Brain -> pick -> one D2H copy - ending in the masked top-k
(ivosw_brain_topk_ragged, agent.candidates = k with agent.skip_annotated) against the same chain ending in ivosw_brain_argmax_ragged
(GPU only), in ONE process.

For K in {1, 8, 32} sessions of T in {30, 100} frames with 1 to 3 objects (cycling), scores and counts on the device, every way runs
ivosw_quality_state_ragged + Brain.forward_ragged (three launches) + its last launch, and ends in the device-to-host copy of
[quality (R) | indices], which synchronises:
  (a) argmax        ivosw_brain_argmax_ragged, K indices                     - the baseline, timed in the same run;
  (k1) (k4) (k16)   ivosw_brain_topk_ragged with skip_annotated, K k indices - k = 1, 4, 16.
Five launches and one copy every way.  A reading is the host clock around REPS such chains (the method of tools/ragged_brain_probe.py: a
launch is what is being exchanged, so the host's time counts), after WARM warm-up chains, the ways ALTERNATING over ROUNDS rounds.  The
report gives each way's median, min .. max and run-to-run spread (max - min), and for every top-k way its difference to (a) against the
larger of the two spreads.  Before timing, top-k with k = 1 and the flag clear is compared with the argmax, and slot 0 of every k with each
other.

usage: python tools/topk_probe.py [--out FILE]        (the report goes to stdout, and to FILE: profiles/topk_probe.txt)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, WARM, REPS = 5, 10, 50
CASES = [(K, T) for T in (30, 100) for K in (1, 8, 32)]
KS = (1, 4, 16)


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


def _legs(dev, agent, K, T):
    import torch
    from ivos_w_amd import _lib as L
    lib = L.lib()
    n_obj = [1 + s % 3 for s in range(K)]
    g = torch.Generator(device=dev).manual_seed(1000 * K + T)
    scores = torch.rand(sum(n_obj) * T, generator=g, device=dev)
    cnt = torch.randint(0, 3, (K * T,), generator=g, device=dev).float()
    lengths, R = [T] * K, K * T
    kept = {}

    def chain(key, k, skip):
        out = torch.zeros(R + K * max(k, 1), dtype=torch.float64, device=dev)
        state = torch.empty(R, 2, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_quality_state_ragged(L.dptr(scores), L.int_array(n_obj), L.int_array(lengths), K, L.dptr(cnt), L.dptr(out),
                                               L.dptr(state), L.stream_ptr(dev)), "quality_state_ragged")
        q, _ = agent.policy_net.forward_ragged(state, lengths)
        if k == 0:
            agent.argmax_ragged(q, lengths, out=out[R:].view(torch.int64))
        else:
            agent.topk_ragged(q, state, lengths, k, skip, out=out[R:].view(torch.int64))
        kept[key] = out.cpu()

    def index(key, k):
        return kept[key][R:].view(torch.int64).view(K, max(k, 1))
    chain("a", 0, False)
    chain("plain", 1, False)
    assert torch.equal(index("a", 0), index("plain", 1)), "top-k with one candidate and no mask differs from the argmax"
    legs = {"a": lambda: chain("a", 0, False)}
    for k in KS:
        legs[f"k{k}"] = (lambda k=k: chain(f"k{k}", k, True))
        legs[f"k{k}"]()
        assert torch.equal(index(f"k{k}", k)[:, 0], index(f"k{KS[0]}", KS[0])[:, 0]) and int(index(f"k{k}", k)[:, :min(k, T)].min()) >= 0
    return legs


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
    say(f"# topk_probe: one process; host clock around chains that end in the D2H copy; {WARM} warm-up chains, {REPS} timed chains per "
        f"reading, {ROUNDS} alternating rounds")
    say(f"# device: {torch.cuda.get_device_name(dev)}")
    say("\n[quality -> state -> ragged Brain -> argmax | masked top-k -> D2H, us per chain over K sessions of T frames]")
    names = {"a": "(a)   argmax_ragged      "}
    names.update({f"k{k}": f"(k{k})".ljust(5) + f" topk_ragged k = {k:2d}  " for k in KS})
    for K, T in CASES:
        say(f" K = {K}, T = {T}, objects 1..3")
        res = _alternate(_legs(dev, agent, K, T), dev)
        med = {k: statistics.median(v) for k, v in res.items()}
        spread = {k: max(v) - min(v) for k, v in res.items()}
        for k in res:
            say(f"  {names[k]}  median {med[k]:8.1f} us   min {min(res[k]):8.1f}   max {max(res[k]):8.1f}   spread {spread[k]:6.1f} us")
        for k in res:
            if k == "a":
                continue
            diff, worst = med[k] - med["a"], max(spread[k], spread["a"])
            verdict = "inside the spread" if abs(diff) <= worst else ("slower by more than the spread" if diff > 0 else "faster by more than the spread")
            say(f"  ({k}) - (a) = {diff:+6.1f} us ({med[k] / med['a']:.3f} x); larger run-to-run spread {worst:.1f} us: {verdict}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
