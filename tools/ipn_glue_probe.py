"""The IPN glue kernels (ivosw_ipn_merge, ivosw_ipn_dilate) against what they replace, at 480p (480 x 854), T = 100 frames, K = 2 and
K = 4 channels (GPU only).

  merge     one interaction's end.  fused: utils_ipn.merge_round - ONE ivosw_ipn_merge call (blend in place, label_u8, label_f32; identity
            channel order, so all_P is a view of all_E) - plus the ONE uint8 copy that brings the labels to the host.  replaced: the
            per-frame torch blend (w * new) + ((1 - w) * old) (3 T small launches) plus To_np_label restated (the whole float estimate
            copied to the host, re-indexed with a fancy-index copy, numpy's argmax).  Host clock around work that ends in a synchronise,
            the two alternating, medians and min .. max over 5 rounds.
  kernel    the merge call alone: HIP events around 10 calls, per call; its bytes (counted from the shapes: all_E read and written,
            prev_E read, 5 B of labels per pixel) over its time, against the 6.3 TB/s float4 copy figure.
  dilate    Dilate_mask for one scribble map with K - 1 objects.  fused: the drop-in (host -> device, ONE ivosw_ipn_dilate launch,
            device -> host) and, for callers that stay on the device, dilate_scribbles on a batch of 8 maps (HIP events, per call).
            replaced: the reference's per-object loop on the host, scipy's binary_dilation standing in for cv2's (cv2 is no dependency).

usage: python tools/ipn_glue_probe.py        (the report goes to stdout)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, H, W, T, COPY_TBS = 5, 480, 854, 100, 6.3


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
    return f"{statistics.median(v):9.2f} {unit}  ({min(v):.2f} .. {max(v):.2f})"


def host_dilate(mask, num_objects):
    """Dilate_mask's loop with scipy's dilation in cv2's place."""
    import numpy as np
    from scipy import ndimage
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    new_mask = -np.ones_like(mask, dtype=np.int64)
    for o in range(num_objects + 1):
        new_mask[ndimage.binary_dilation(mask == o, structure=cross, iterations=2)] = o
    return new_mask


def main():
    import numpy as np
    import torch
    from ivos_w_amd.utils import utils_ipn as ui
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    print(f"IPN glue probe: {H} x {W}, T = {T}, {ROUNDS} rounds, medians (min .. max)")
    for K in (2, 4):
        all_E = torch.softmax(torch.randn(1, K, T, H, W, generator=g), 1).to(dev)
        prev_E = torch.softmax(torch.randn(1, K, T, H, W, generator=g), 1).to(dev)
        _, _, weight = ui.Get_weight(40, [10, 75], T, at_least=5)
        index = list(range(K))
        store = ui.IpnStore(T, K, H, W, dev, all_E=all_E)
        keep = {}

        def fused():
            keep["masks"], keep["all_P"] = ui.merge_round(all_E, prev_E, weight, None, store)
            keep["labels"] = store.labels_u8.cpu().numpy()

        def replaced():
            for f in range(T):
                all_E[:, :, f] = (weight[f] * all_E[:, :, f]) + ((1 - weight[f]) * prev_E[:, :, f])
            sh_E = all_E[0].data.cpu().numpy()
            inv_index = [index.index(i) for i in range(K)]
            keep["labels"] = np.argmax(sh_E[inv_index], axis=0).astype(np.uint8)
            keep["all_P"] = all_E[0].transpose(1, 0)

        r = _alternate({"fused": fused, "replaced": replaced}, lambda fn: _wall(fn, dev), 1)
        print(f"merge, K = {K}:  fused (one call + one uint8 copy) {_fmt(r['fused'], 'ms')}   "
              f"torch blend loop + host To_np_label {_fmt(r['replaced'], 'ms')}")
        print(f"    the replaced path copies {K * T * H * W * 4 / 1e6:.0f} MB to the host, the fused one {T * H * W / 1e6:.0f} MB")

        def call():
            ui.merge_round(all_E, prev_E, weight, None, store)

        call()
        k = [_events(call, 10, dev) for _ in range(ROUNDS)]
        moved = 3 * K * T * H * W * 4 + 5 * T * H * W
        us = statistics.median(k)
        print(f"kernel, K = {K}:  {_fmt(k, 'us')} per merge call; it moves {moved / 1e9:.2f} GB -> {moved / us / 1e6:.2f} TB/s at the median, "
              f"{100 * moved / us / 1e6 / COPY_TBS:.0f} % of the {COPY_TBS} TB/s float4 copy figure")
        del all_E, prev_E, store, keep

        rng = np.random.default_rng(K)
        mask = np.where(rng.random((H, W)) < 0.01, rng.integers(0, K, (H, W)), -1)
        r = _alternate({"fused": lambda: ui.Dilate_mask(mask, K - 1, device=dev), "replaced": lambda: host_dilate(mask, K - 1)},
                       lambda fn: _wall(fn, dev), 2)
        batch = torch.from_numpy(np.stack([mask] * 8).astype(np.int8)).to(dev)
        d = [_events(lambda: ui.dilate_scribbles(batch, K - 1), 50, dev) for _ in range(ROUNDS)]
        print(f"dilate, {K - 1} object(s):  drop-in (copy in, one launch, copy out) {_fmt(r['fused'], 'ms')}   host loop (scipy) {_fmt(r['replaced'], 'ms')}")
        print(f"    dilate_scribbles on the device, 8 maps in one launch: {_fmt(d, 'us')} per call")


if __name__ == "__main__":
    main()
