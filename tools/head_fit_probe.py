#!/usr/bin/env python
"""Times one epoch of the head fit (M = 4096 rows, B = 32: 128 steps) on the GPU: ivosw_head_fit with 1 fit and with 32 fits in one
launch, against the same loop written with torch ops on the same GPU (nn.Linear, autograd, clamp_, optim.SGD, one .item() per step as the
reference's meters take it).  The legs alternate; medians of 5 rounds with min .. max, host clock around a synchronised call.

    python tools/head_fit_probe.py [out.txt]          (default profiles/head_fit_probe.txt)
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ivos_w_amd  # noqa: E402,F401
from ivos_w_amd import _lib as L  # noqa: E402

M, B, C, ROUNDS = 4096, 32, 2048, 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "head_fit_probe.txt")
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    feat = torch.from_numpy(np.maximum(rng.standard_normal((M, C)), 0).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(0, 1, M).astype(np.float32)).to(dev)
    valid = torch.ones(M, dtype=torch.uint8, device=dev)
    steps = M // B
    order = rng.permutation(M).astype(np.int32).reshape(steps, B)
    lr, mom, wd = 5e-6, 0.9, 5e-4
    lib, st = L.lib(), L.stream_ptr(dev)

    def device_leg(k):
        order_d = torch.from_numpy(np.broadcast_to(order, (k, steps, B)).copy()).to(dev)
        lr_d = torch.full((k, steps), lr, dtype=torch.float32, device=dev)
        w, b = torch.zeros(k, C, device=dev), torch.zeros(k, device=dev)
        bw, bb, gw, gb = torch.zeros(k, C, device=dev), torch.zeros(k, device=dev), torch.zeros(k, C, device=dev), torch.zeros(k, device=dev)
        taken, log = torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(k, steps, 3, device=dev)
        f = lambda v: (ctypes.c_float * k)(*([v] * k))
        i = lambda v: (ctypes.c_int * k)(*([v] * k))

        def run():
            L.check(lib.ivosw_head_fit(L.dptr(feat), L.dptr(target), L.dptr(valid), M, L.dptr(order_d), L.dptr(lr_d), k, steps, B, f(mom), f(wd),
                                       i(1), i(0), L.dptr(w), L.dptr(b), L.dptr(bw), L.dptr(bb), L.dptr(gw), L.dptr(gb), L.dptr(taken),
                                       L.dptr(log), st), "head_fit")
            return log.cpu()                                        # the epoch's one copy
        return run

    def torch_leg():
        lin = torch.nn.Linear(C, 1).to(dev)
        opt = torch.optim.SGD(lin.parameters(), lr=lr, momentum=mom, weight_decay=wd)
        order_t = torch.from_numpy(order.astype(np.int64)).to(dev)

        def run():
            tot = 0.0
            for s in range(steps):
                idx = order_t[s]
                e = lin(feat[idx]).view(-1) - target[idx]
                ok = valid[idx] != 0
                loss = (e * e)[ok].sum() / ok.sum()
                opt.zero_grad()
                loss.backward()
                for p in lin.parameters():
                    p.grad.data.clamp_(-1, 1)
                opt.step()
                tot += loss.item()
            return tot
        return run

    legs = [("ivosw_head_fit, 1 fit", device_leg(1), 1), ("ivosw_head_fit, 32 fits in one launch", device_leg(32), 32),
            ("torch ops (nn.Linear, autograd, clamp_, SGD), 1 fit", torch_leg(), 1)]
    for _, run, _ in legs:                                          # warm-up: code objects, allocator, autograd
        run()
    times = {name: [] for name, _, _ in legs}
    for _ in range(ROUNDS):
        for name, run, _ in legs:                                   # the legs alternate
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) * 1e3)
    lines = [f"head fit, one epoch: M = {M} rows, B = {B}, {steps} steps; host clock around a synchronised call, medians of {ROUNDS} "
             f"alternating rounds (min .. max)", f"device: {torch.cuda.get_device_name(dev)}"]
    for name, _, k in legs:
        t = np.array(times[name])
        lines.append(f"{name:55s} {np.median(t):9.3f} ms ({t.min():.3f} .. {t.max():.3f})   {np.median(t) * 1e3 / steps:8.2f} us per step"
                     + (f"   {np.median(t) * 1e3 / steps / k:8.2f} us per step and fit" if k > 1 else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
