"""The ATNet epilogue (ivosw_atnet_epilogue) against the torch op sequence it replaces, at 480p as ATNet pads it (GPU only).

480 x 854 padded to 512 x 864 (pads 16, 16, 5, 5: up to the next multiple of 32, a whole 32 where the extent already is one, so that
both trailing pads are positive - the reference's crop [hpad1:-hpad2] needs that).  wpad1 = 5 puts the window off the 16-byte grid of
the padded rows: the kernel that runs is the one with vector loads and element window stores.

  frame         per propagated frame, 1 and 3 objects: the fused call (sigmoid, blend in place, prob_pad, store slot, both label planes)
                against torch.sigmoid, the channel slice, two scalar multiplies, the add and the indexed store - which leave the labels,
                the crop and the zero channel to the end of the interaction.  HIP events around 200 calls, the two alternating, medians
                and min .. max over 5 rounds; and the fused call's bytes (counted from the shapes) over its time.
  interaction   the end-of-interaction part of a 100-frame session against nothing at all: combine_masks_with_batch (argmax, per object an
                equality, a threshold, a product, a masked store), the crop, the host copy and float64 cast, and torch.cat([zeros, map], 1)
                cropped - against the ONE uint8 copy the fused path has left.  Host clock around work that ends in a synchronise.

usage: python tools/atnet_epilogue_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, CALLS, H, W, PADS, N_VIDEO, TH = 5, 200, 480, 854, (16, 16, 5, 5), 100, 0.8
PH, PW = H + PADS[0] + PADS[1], W + PADS[2] + PADS[3]


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
    return f"{statistics.median(v):9.1f} {unit}  ({min(v):.1f} .. {max(v):.1f})"


def combine_masks_with_batch(prob, n_obj, th):
    """The op sequence of the clone's combine: an argmax, then per object an equality, a threshold, a product and a masked store."""
    import torch
    am = torch.argmax(prob, dim=1, keepdim=True)
    out = torch.zeros_like(am, dtype=torch.float32)
    for o in range(n_obj):
        hit = (am == o).float() * (prob[:, o:o + 1] > th).float()
        out[hit > 0] = o + 1
    return out


def main():
    import numpy as np
    import torch
    from ivos_w_amd.utils import utils_atnet as ua
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    print(f"ATNet epilogue probe: {H} x {W} padded to {PH} x {PW}, pads {PADS}, {ROUNDS} rounds, medians (min .. max)")
    for n_obj in (1, 3):
        n = 4                                             # frames of the per-frame legs: enough to walk off the L2 between calls
        pm = torch.rand(n, n_obj, PH, PW, generator=g).to(dev)
        logits = (torch.randn(n_obj, 1, PH, PW, generator=g) * 3).to(dev)
        store = ua.AtnetStore(n, n_obj, H, W, dev)
        alpha = 0.75
        state = {"t": 0}

        def fused():
            state["t"] = (state["t"] + 1) % n
            ua.atnet_epilogue(logits, pm, state["t"], PADS, TH, store, alpha=alpha)

        def torch_ops():
            state["t"] = (state["t"] + 1) % n
            prob = torch.sigmoid(logits)
            p = prob[:, 0].detach()
            p = (alpha * p) + ((1 - alpha) * pm[state["t"]])
            pm[state["t"]] = p

        r = _alternate({"fused": fused, "torch": torch_ops}, lambda fn: _events(fn, CALLS, dev), 20)
        plane = n_obj * PH * PW * 4
        moved = 4 * plane + n_obj * H * W * 4 + H * W * 5  # logits + map read, map + prob_pad written; slot, u8 and f32 labels written
        us = statistics.median(r["fused"])
        print(f"frame, {n_obj} object(s):  fused {_fmt(r['fused'], 'us')}   torch sequence {_fmt(r['torch'], 'us')}")
        print(f"    fused call moves {moved / 1e6:.2f} MB -> {moved / us / 1e6:.2f} TB/s at the median (host launch path included)")

        # the end of a 100-frame interaction
        del pm, store
        pm = torch.rand(N_VIDEO, n_obj, PH, PW, generator=g).to(dev)
        store = ua.AtnetStore(N_VIDEO, n_obj, H, W, dev, probs=False)
        h1, h2, w1, w2 = PADS
        keep = {}

        def torch_end():
            keep["masks"] = combine_masks_with_batch(pm, n_obj, TH)[:, 0, h1:-h2, w1:-w2].cpu().numpy().astype(np.float64)
            keep["all_P"] = torch.cat([torch.zeros_like(pm[:, 0:1]), pm], 1)[:, :, h1:-h2, w1:-w2]

        def fused_end():
            keep["masks"] = store.labels_u8.cpu().numpy().astype(np.float64)

        r = _alternate({"fused": fused_end, "torch": torch_end}, lambda fn: _wall(fn, dev), 2)
        print(f"interaction end, {N_VIDEO} frames, {n_obj} object(s):  fused (one uint8 copy + cast) {_fmt(r['fused'], 'ms')}   "
              f"torch (combine, crop, host copy, zero-channel cat) {_fmt(r['torch'], 'ms')}")
        print(f"    the cat alone allocates and writes {(n_obj + 1) * N_VIDEO * PH * PW * 4 / 1e6:.0f} MB")
        del pm, store, keep


if __name__ == "__main__":
    main()
