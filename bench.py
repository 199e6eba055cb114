#!/usr/bin/env python
"""bench.py — throughput of the IVOS-W hot path on MI355X (one process per GPU).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
                                                             (N > 1: launched by torch.distributed.run, or plainly — it then
                                                              starts torch.distributed.run as a child, one rank per GPU)

A plain run measures the headline only: set-up, warm-up, K timed steps, one JSON line with `metric`, `value`, `unit`,
`higher_is_better`, `dtype` and `ms_per_step` (+ the run's config).  `--full` adds everything else described below (the oracle
check, roofline, sustained rate, the DQN leg, the fp32 / bf16x3 modes, front end, recommend_frame, J&F, seg epilogue, CPU baselines,
the data-parallel and P2P legs); those records exist only in a --full line.  `--dump-outputs DIR` writes what the timed path returned in
its last step as float32 .npy files (`scores` [B, 1] of the assessment; `policy_params` / `target_params` of the DQN workload); the
inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.

Default workload = BASELINE.json configs[1]: the assessment CNN (AssessNet.forward) on a batch of 256
synthetic 480p (frame, mask) pairs per GPU, bf16 operands / fp32 accumulate, inputs resident in HBM when
the clock starts.  One "step" = one AssessNet.forward over the batch.  `value` = assessed frames/s over all
ranks (frames are independent: weak scaling, no data-path collective).

A --full line also carries, as `dqn`, the second half of BASELINE's metric: Double-DQN agent steps/s
(configs[2]/[3]: replay 50k transitions, minibatch 128 per GPU, T=25; device-resident replay gather ->
3 forwards + loss + BPTT -> [RCCL all-reduce of the 724 KB gradient arena when N>1] -> clamp+Adam ->
target-sync coin flip).  `--workload dqn` makes that the headline `value` instead.

Timing: W warm-up steps, extended until at least --min-warm-s seconds of the same work have run (the shader clock falls from
2.4 to ~1.6 GHz under sustained MFMA load: a cold 80 ms window is not a steady-state figure), then EXACTLY K steps between
barrier + synchronize pairs.  With no flags K = 250 (> 1 s of work).  `sustained` repeats the measurement over a window of
at least 1 s whatever K was.

roofline: dominant kernel family = the tower's contraction kernels, conv_igemm* | conv1x1_wide* | conv3x3_patch* (layer by layer), stem_pool* and bneck* (whole
bottlenecks / stage runs fused) (bound: bf16 MFMA, 2.5 PFLOP/s dense).  achieved = algorithmic conv FLOPs per launch /
average launch duration, where the family's time is measured INSIDE the timed region with one HIP-event pair per forward pass
on the launch stream (ivosw_profile_span_*: stem .. last res5 kernel; the bbox / ROI kernels before and the pool+fc kernel after
are outside the pair), so family time <= ms_per_step by construction and nothing is bracketed per launch.
`roofline.traffic`: HBM bytes per launch of that family MEASURED IN THIS RUN (N = 1): after the timed region the same forward is
re-run in two child processes under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (live_traffic(); counters only, ~10 s); if
rocprofv3 is missing or a child fails, the committed summary of the same passes (profiles/pmc_traffic_latest.json) is quoted and
`traffic_source` says so.
`roofline.reference_gemm` (round 6; was `attainable`): what this build's plain-HIP 256 x 256 8-phase contraction (the CDNA4 guide's template,
ivos-w_amd/csrc/gemm_8phase.h) reached on uniform random bf16 in a COMMITTED run (profiles/r06_gemm_8phase_v1/v2.txt: 1.35 - 1.37 PFLOP/s at
4096^3, 1.29 - 1.35 at 8192^3, K loops 1.24 - 1.55) - a reference measurement from one box, NOT re-measured in this run and not a property
of the chip (the guide reports 1.75 - 1.9 PFLOP/s with inline asm) - and the achieved tower rate as a fraction of it, beside `frac` against
the 2.5 PFLOP/s peak.
`dqn.dp_critical_path` (round 5, N = 1): the DQN step re-run in a child through the N > 1 branch on nccl with ONE rank (`--gpus 1 --force-dist`:
process group, all-reduce of the gradient arena in every step, clamp + Adam with 1/world) against the fused single-GPU step.
`dqn.collectives` (N > 1): `backend` = the step timed through torch.distributed's all-reduce (= `dqn.value`: the product default), with the process
group's own world size and backend string; `p2p` = the one-shot xGMI peer-to-peer all-reduce fused with clamp + Adam (opt-in in the product), attempted by
default as the LAST act of the run - after every other number of the line exists - under LineGuard: a watchdog child holds the finished line and prints it
if the process dies inside that leg; `dqn.scaling_vs_1gpu` = whole-job steps/s over the committed single-GPU rate.  IVOSW_BENCH_P2P=0 skips the leg.
`checked`: after the timed region a sample of the B=256 scores is compared with the oracle on the CPU (and the fp32 parity
mode, which is also timed: `fp32`); the line is not printed if they disagree.  cpu_baseline: torch-CPU restatements of the
reference path (kind "port") on bounded samples, rank 0, N=1 only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ivos_w_amd import _lib as L            # noqa: E402
from ivos_w_amd import synth                # noqa: E402

GFLOP_PER_FRAME = 10.779365376              # 5 389 682 688 MAC x 2, conv stack + fc
CONV_LAUNCHES_PER_FRAME_CHUNK = 54           # stem + 53 tower convs, per chunk
PEAK_BF16_TFLOPS = 2500.0                    # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
# A committed REFERENCE measurement (one box, round 6), not a roof of the chip and not re-measured per run: the plain-HIP 256 x 256 8-phase
# contraction of the CDNA4 guide as re-derived in ivos-w_amd/csrc/gemm_8phase.h, uniform random bf16 (profiles/r06_gemm_8phase_v1.txt, _v2.txt):
# whole GEMM at 4096^3 / 8192^3, and the K loop alone at the tower's K-heavy layer shapes (768 ... 2304 deep).  Round 5 quoted its own
# one-wave-per-SIMD probe here (1 100 / 1 310) as "the attainable roof"; the 8-phase schedule beats it by 20 - 25 % with the same builtins.
REFERENCE_GEMM_BF16_TFLOPS = {"gemm_4096": 1365.0, "gemm_8192": 1349.0, "k_loop_tower_shapes": [1240.0, 1470.0]}
PEAK_F32_TFLOPS = 157.3
BF16_SCORE_RTOL = 4e-3                      # the bf16 mode's stated tolerance (tests/test_gpu_assess.py)
DQN_GFLOP_PER_STEP = 10.5                    # 3 forwards + backward at B=128, T=25


class AD(dict):
    __getattr__ = dict.__getitem__


# the single-GPU DQN rate the N > 1 runs are scaled against (dqn.scaling_vs_1gpu): a committed measurement, not re-measured in an N > 1 run
DQN_1GPU_REF = {"steps_per_sec": 5470.0, "us_per_step": 182.7, "source": "BENCH_r05.json / profiles/r05_bench_final.json.log: fused single-GPU step, minibatch 128, replay 50 000"}


def agent_cfg():
    return AD(phase="train", data=AD(subset="train"),
              agent=AD(memory_size=100000, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                       update_rate=0.05, lr=5e-6, weight_decay=5e-4))        # configs/config.yaml agent block


def dist_setup(n):
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if n > 1 and world != n:
        raise SystemExit(f"--gpus {n} under a launcher with WORLD_SIZE={world}: the two must agree")
    # --backend gloo + IVOSW_BENCH_SAME_DEVICE=1: every rank on cuda:0 with host-staged collectives — the only way to run the
    # multi-rank code path on a one-GPU box (tests/test_gpu_dist.py); the driver's 2/4/8-GPU runs use nccl = RCCL over xGMI
    if os.environ.get("IVOSW_BENCH_SAME_DEVICE") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or FORCE_DIST[0]:
        import torch.distributed as dist_
        if world == 1:                       # --force-dist: a process group of one rank, through the same backend
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if BACKEND[0] == "nccl":
            dist_.init_process_group("nccl", device_id=dev)
        else:
            dist_.init_process_group(BACKEND[0])
        dist = dist_
    return rank, world, dev, dist


BACKEND = ["nccl"]
FORCE_DIST = [False]     # --force-dist: N = 1 through the N > 1 branch (process group of one rank, the collective in every DQN step)


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def reduce_scalar(dist, value, op, dev):
    """max / min of a host scalar over the ranks (a CPU tensor under gloo, a device tensor under RCCL)."""
    t = torch.tensor([value], dtype=torch.float64, device=dev if BACKEND[0] == "nccl" else "cpu")
    dist.all_reduce(t, op=op)
    return float(t.item())


def allreduce_grads(dist, flat_grad):
    if BACKEND[0] == "nccl":
        dist.all_reduce(flat_grad)                      # RCCL over xGMI
    else:
        from ivos_w_amd import parallel
        parallel.allreduce_grads(flat_grad)             # gloo: staged through host memory


def timed(fn, steps, warmup, dev, dist, min_warm_s=0.0, before=None, after=None):
    """W warm-up steps (extended to min_warm_s seconds of the same work), then exactly `steps` steps between barrier +
    synchronize pairs; the max over ranks.  `before` / `after` run inside the bracket's host side but enqueue no kernels."""
    t_w = time.perf_counter()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    def warm_enough():
        el = time.perf_counter() - t_w
        if dist is not None:                   # every rank must take the same decision (the step may contain a collective)
            el = reduce_scalar(dist, el, dist.ReduceOp.MIN, dev)
        return el >= min_warm_s
    while min_warm_s > 0 and not warm_enough():
        for _ in range(max(1, warmup)):
            fn()
        torch.cuda.synchronize(dev)
    if before is not None:
        before()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if after is not None:
        after()
    if dist is not None:
        dt = reduce_scalar(dist, dt, dist.ReduceOp.MAX, dev)
    return dt


def dump_outputs(path, arrays, rank, world):
    """--dump-outputs: the arrays the timed path returned in its last step, one float32 .npy per array (per rank when N > 1)."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, (name if world == 1 else f"{name}_rank{rank}") + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def build_assess(args, rank, dev):
    from ivos_w_amd.models.assessment import AssessNet
    net = AssessNet(precision=args.precision, chunk=args.chunk)
    sd = synth.assessnet_state_dict(0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net.to(dev).eval()
    # SURVEY §8(d) A2 inputs; generated per 32 frames to bound host memory, rank-offset seed
    tf = torch.empty(args.batch, 3, 480, 854, dtype=torch.float32, device=dev)
    tp = torch.empty(args.batch, 480, 854, dtype=torch.float32, device=dev)
    for i in range(0, args.batch, 32):
        n = min(32, args.batch - i)
        a, b = synth.assess_inputs(n, seed=1234 + 1000 * rank + i)
        tf[i:i + n].copy_(torch.from_numpy(a))
        tp[i:i + n].copy_(torch.from_numpy(b))
    return net, tf, tp


def check_scores(scores, tf, tp, precision, pick):
    """A sample of the timed batch against the oracle (CPU restatement of the reference) — outside the timed region."""
    from oracle import assess_oracle as ao          # checker only
    sd = ao.to_torch_sd(synth.assessnet_state_dict(0))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = ao.assess_forward(sd, tf[pick].cpu().numpy(), tp[pick].cpu().numpy()).reshape(-1)
    got = scores.reshape(-1)[pick].cpu().numpy()
    tol = BF16_SCORE_RTOL if precision == "bf16" else 1e-4
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    if not (err <= tol):
        raise SystemExit(f"bench.py: scores of the timed batch disagree with the oracle (worst rel err {err:.3e} > {tol}): no line printed")
    return {"frames": len(pick), "worst_rel_err": float(f"{err:.3e}"), "tolerance": tol, "against": "oracle/assess_oracle.py (torch-CPU restatement of AssessNet.forward)"}


def dqn_dp_critical_path(single_us, timeout_s=150):
    """The left-hand side of DESIGN section 6's scaling budget, measured: the SAME DQN step run in a child process
    through the N > 1 branch on the backend that the multi-GPU job uses (`--gpus 1 --force-dist`: a process group of one rank on nccl = RCCL;
    gradients -> dist.all_reduce of the 724 KB arena on the compute stream -> clamp + Adam with 1/world, plain launches), against the
    fused single-GPU step of this run.  Their difference is what data parallelism adds to a step before any wire time: the launch gaps of
    the un-fused structure, RCCL's kernel for a one-rank communicator and the separate clamp + Adam.  None when the child fails."""
    import subprocess
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--workload", "dqn", "--steps", "800", "--warmup", "50",
           "--no-cpu-baseline", "--full"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout_s)
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        dp_us = float(line["collectives"]["backend"]["us_per_step"])
    except Exception:
        return None
    return {"us_per_step_through_the_collective_branch": dp_us, "us_per_step_fused_single_gpu": round(single_us, 1),
            "added_by_the_data_parallel_structure_us": round(dp_us - single_us, 1),
            "budget_us_for_6x_at_8_gpus": round(single_us * (8.0 / 6.0 - 1.0), 1),
            "how": "child run `bench.py --gpus 1 --force-dist --workload dqn`: process group of ONE rank on nccl (RCCL), all-reduce of the 724 KB "
                   "gradient arena + clamp + Adam as plain launches; wire time between GPUs is NOT in it (no second GPU on this box)"}


def live_traffic(family, launches_per_pass, conv_ms, passes=3, timeout_s=75):
    """roofline.traffic measured in THIS run: the same forward (batch 256, bf16, default chunk) is re-run in two child processes
    under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes, counters only - no trace domains), after the
    timed region, and the per-kernel counters of the tower family are summed exactly as tools/pmc_summary.py does for the
    committed profiles (KiB units, FETCH_SIZE x 2 on gfx950).  Returns None (the committed summary stays quoted) when
    rocprofv3 is missing, a child fails or times out, or the launch count does not match the timed run."""
    import glob
    import importlib.util
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):      # never nest profilers
        return None
    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(ROOT, "tools", "pmc_summary.py"))
    pmc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pmc)
    fams = [f.strip("*") for f in family.split("|")]
    tmp = tempfile.mkdtemp(prefix="ivosw_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    got = {}
    t0 = time.perf_counter()
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [prof, "--pmc", counter, "-d", d, "-o", "c", "--output-format", "csv", "--", sys.executable, os.path.join(ROOT, "bench.py"),
                   "--tower-only", "--steps", str(passes - 1), "--warmup", "1"]
            child = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
            try:
                child.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(child.pid, 9)                    # the profiler AND the python it started (own session: exact group)
                child.communicate()
                return None
            r = child
            csvs = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not csvs:
                if os.environ.get("IVOSW_BENCH_DEBUG"):
                    print(f"live_traffic: child rc {r.returncode}, csvs {csvs}", file=sys.stderr)
                return None
            agg = pmc.load(csvs[0], counter)
            n = sum(v[0] for k, v in agg.items() if any(f in k for f in fams))
            kib = sum(v[1] for k, v in agg.items() if any(f in k for f in fams))
            got[counter] = (n, kib * 1024.0)
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    (nf, rd), (nw, wr) = got["FETCH_SIZE"], got["WRITE_SIZE"]
    rd *= 2.0                                              # gfx950: FETCH_SIZE reports half the bytes of wide streaming reads
    if nf != nw or nf != launches_per_pass * passes:
        if os.environ.get("IVOSW_BENCH_DEBUG"):
            print(f"live_traffic: launches {nf} / {nw} against {launches_per_pass} x {passes}", file=sys.stderr)
        return None
    per_pass = (rd + wr) / passes
    return {"traffic": round((rd + wr) / nf), "traffic_bytes_per_step": round(per_pass),
            "traffic_read_write_GB_per_step": [round(rd / passes / 1e9, 3), round(wr / passes / 1e9, 3)],
            "traffic_source": f"measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two separate child runs of `bench.py --tower-only`, {passes} forward passes "
                              f"each, {nf} launches of the family; FETCH_SIZE x2 gfx950 correction, KiB units), {round(time.perf_counter() - t0)} s",
            "hbm_GBps_of_family": round(per_pass / (conv_ms * 1e-3) / 1e9, 1) if conv_ms > 0 else None}


def dqn_live_traffic(timeout_s=60):
    """dqn.roofline.traffic measured in THIS run: the DQN loop re-run in two child processes under `rocprofv3 --pmc
    FETCH_SIZE` / `--pmc WRITE_SIZE` (counters only), every kernel summed, divided by the number of steps (= launches of the encoder
    kernel, one per step).  KiB units, FETCH_SIZE x 2 on gfx950 (MI355X_MICROARCH.md, HBM).  None when rocprofv3 is missing or a child fails."""
    import glob
    import importlib.util
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(ROOT, "tools", "pmc_summary.py"))
    pmc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pmc)
    tmp = tempfile.mkdtemp(prefix="ivosw_pmc_dqn_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    got, per_kernel = {}, {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [prof, "--pmc", counter, "-d", d, "-o", "c", "--output-format", "csv", "--", sys.executable, os.path.join(ROOT, "bench.py"),
                   "--workload", "dqn", "--steps", "96", "--warmup", "8", "--min-warm-s", "0", "--dqn-mode", "plain", "--no-cpu-baseline", "--full"]
            child = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
            try:
                child.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(child.pid, 9)
                child.communicate()
                return None
            csvs = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if child.returncode != 0 or not csvs:
                return None
            agg = pmc.load(csvs[0], counter)
            steps = sum(v[0] for k, v in agg.items() if "enc_fused" in k)
            if steps <= 0:
                return None
            scale = 2.0 if counter == "FETCH_SIZE" else 1.0
            got[counter] = sum(v[1] for v in agg.values()) * 1024.0 * scale / steps
            for k, v in agg.items():
                per_kernel[k.split("(")[0][-48:]] = per_kernel.get(k.split("(")[0][-48:], 0.0) + v[1] * 1024.0 * scale / steps
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    top = sorted(per_kernel.items(), key=lambda kv: -kv[1])[:6]
    return {"traffic": round(got["FETCH_SIZE"] + got["WRITE_SIZE"]), "traffic_read_write_MB_per_step": [round(got["FETCH_SIZE"] / 1e6, 1), round(got["WRITE_SIZE"] / 1e6, 1)],
            "algorithmic_bytes_per_step": 7.0e6, "traffic_top_kernels_MB_per_step": {k: round(v / 1e6, 1) for k, v in top},
            "traffic_source": "measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two child runs of `bench.py --workload dqn`, every kernel, "
                              "per step = per launch of the encoder kernel; FETCH_SIZE x2 gfx950 correction, KiB units)"}


def bench_front(args, dev, tf, tp):
    """the assessment front end (mask -> box, ROI crop-resize + normalise) is HBM-bound - timed on its own through
    the two C-ABI entry points on the timed batch; algorithmic bytes = `tp` once for the box pass, and for the crop the source
    pixels inside each sample's box (3 frame planes + the mask plane, fp32) once + the ROI tile written once."""
    lib = L.lib()
    B, H, W = tp.shape
    code = {"bf16": L.BF16, "fp32": L.F32, "bf16x3": L.F32X3}[args.precision]
    yxhw = torch.empty(B, 4, device=dev, dtype=torch.float32)
    scratch = torch.empty(B * 4, device=dev, dtype=torch.int32)
    roi = torch.empty(B, 256, 256, 4, device=dev, dtype=torch.bfloat16 if args.precision == "bf16" else torch.float32)
    st = L.stream_ptr(dev)

    def bbox():
        L.check(lib.ivosw_mask_bbox(L.dptr(tp), B, H, W, L.dptr(yxhw), L.dptr(scratch), st), "mask_bbox")

    def crop():
        L.check(lib.ivosw_roi_sample(L.dptr(tf), L.dptr(tp), L.dptr(yxhw), B, H, W, code, L.dptr(roi), st), "roi_sample")
    out = {}
    for name, fn in (("bbox", bbox), ("roi", crop)):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 30
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out[name] = e0.elapsed_time(e1) * 1e3 / n
    box = yxhw.cpu().numpy().astype(np.float64)
    hh = np.clip(np.minimum(box[:, 0] + box[:, 2] / 2, H) - np.maximum(box[:, 0] - box[:, 2] / 2, 0), 0, H)      # (y, x) = box centre
    ww = np.clip(np.minimum(box[:, 1] + box[:, 3] / 2, W) - np.maximum(box[:, 1] - box[:, 3] / 2, 0), 0, W)
    bytes_bbox = float(B) * H * W * 4
    bytes_roi = float(np.sum(hh * ww) * 4 * 4) + float(B) * 256 * 256 * 4 * roi.element_size()
    us = out["bbox"] + out["roi"]
    ach = (bytes_bbox + bytes_roi) / (us * 1e-6) / 1e9
    return {"kernels": "bbox_scan|bbox_finalize|roi_sample", "us_per_step": round(us, 1), "bbox_us": round(out["bbox"], 1), "roi_us": round(out["roi"], 1),
            "roofline": {"bound": "hbm", "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4),
                         "bbox_GBps": round(bytes_bbox / (out["bbox"] * 1e-6) / 1e9, 1), "roi_GBps": round(bytes_roi / (out["roi"] * 1e-6) / 1e9, 1),
                         "note": "algorithmic bytes: tp read once by the box pass; box pixels of 3 frame planes + mask (fp32) read once and the 256x256x4 tile written once by the crop (the box is clipped to the frame)"}}


def _read_power_w():
    """Average socket power in W from the amdgpu hwmon node (power1_average / power1_input, microwatts), or None."""
    import glob
    for pat in ("/sys/class/drm/card*/device/hwmon/hwmon*/power1_average", "/sys/class/drm/card*/device/hwmon/hwmon*/power1_input"):
        for path in sorted(glob.glob(pat)):
            try:
                v = float(open(path).read().strip())
                if v > 0:
                    return v / 1e6
            except (OSError, ValueError):
                pass
    return None


def measure_clock_and_power(step, dev, passes=12, spin_us=2500):
    """Shader clock and socket power UNDER the measured load: while `passes` more forward passes run back to back, a one-wave probe
    kernel on a side stream spins for `spin_us` (~ one pass: the clock differs from kernel to kernel, so the window must cover the pass) and reports (shader cycles by s_memtime) / (100 MHz wall ticks by
    s_memrealtime) -> MHz; the hwmon power node is read from the host between passes.  The probe occupies one wave slot of one CU."""
    lib = L.lib()
    side = torch.cuda.Stream(device=dev)
    out = torch.zeros(passes, 2, dtype=torch.int64, device=dev)
    for _ in range(3):
        step()
    torch.cuda.synchronize(dev)
    watts = []
    for i in range(passes):
        L.check(lib.ivosw_clock_probe(out[i].data_ptr(), int(spin_us), ctypes.c_void_p(side.cuda_stream)), "clock_probe")
        step()
        w = _read_power_w()
        if w is not None:
            watts.append(w)
    torch.cuda.synchronize(dev)
    o = out.cpu().numpy().astype(np.float64)
    mhz = o[:, 0] / np.maximum(o[:, 1], 1.0) * 100.0
    rec = {"sclk_mhz": round(float(np.median(mhz)), 1), "sclk_mhz_min_max": [round(float(mhz.min()), 1), round(float(mhz.max()), 1)],
           "sclk_source": f"s_memtime / s_memrealtime of a one-wave probe kernel ({int(spin_us)} us windows = one pass each) running beside 12 back-to-back forward passes (ivosw_clock_probe); "
                          "a PASS AVERAGE: MFMA-dense kernels pull the clock down (res4 / res3 block kernels run at ~1.45 - 1.55 GHz by their own cycle stamps), lighter ones run above it",
           "power_w": round(float(np.mean(watts)), 1) if watts else None,
           "power_source": "amdgpu hwmon power1_average, read between the passes" if watts else "no readable hwmon power node on this box"}
    return rec


def bench_assess(args, rank, world, dev, dist):
    net, tf, tp = build_assess(args, rank, dev)
    lib = L.lib()
    out = {}

    def step():
        out["s"] = net(tf, tp)
    tot, spans, cnt = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_int(0)
    # the tower's span timing (roofline) records its event pairs inside the timed region: --full only
    dt = timed(step, args.steps, args.warmup, dev, dist, args.min_warm_s,
               before=(lambda: lib.ivosw_profile_span_start()) if args.full else None,
               after=(lambda: lib.ivosw_profile_span_stop(ctypes.byref(tot), ctypes.byref(spans), ctypes.byref(cnt))) if args.full else None)
    assert torch.isfinite(out["s"]).all()
    scores = out["s"].clone()
    fps = args.total_batch * args.steps / dt
    if args.full:
        split = bool(lib.ivosw_assess_split({"bf16": L.BF16, "fp32": L.F32, "bf16x3": L.F32X3}[args.precision], args.batch, args.chunk or 0))
        # one span per ROI chunk; with the two-stream split of the batch the two halves' spans form one group per forward pass
        assert spans.value == (args.steps if split else args.steps * -(-args.batch // net_chunk(args))), (spans.value, args.steps)
        conv_ms = tot.value / args.steps
        launches = cnt.value // args.steps
        # sustained: the same measurement over >= 1 s, whatever K was
        sus = None
        if args.min_warm_s <= 0:
            sus = {"value": None, "note": "skipped (--min-warm-s 0: profiling run)"}
        elif dt < 1.0:
            n = int(1.2 / (dt / args.steps)) + 1
            sdt = timed(step, n, 0, dev, dist)
            sus = {"value": round(args.total_batch * n / sdt, 1), "steps": n, "seconds": round(sdt, 3)}
        else:
            sus = {"value": round(fps, 1), "steps": args.steps, "seconds": round(dt, 3)}
    if args.layer_report and rank == 0:
        L.tune_set(b"STREAMS2", 0)                  # per-launch events: one stream, or the halves' kernels time each other
        lib.ivosw_profile_start()
        for _ in range(3):
            step()
        L.tune_set(b"STREAMS2", 1)
        buf = ctypes.create_string_buffer(1 << 16)
        lib.ivosw_profile_report(buf, len(buf))
        t2, c2 = ctypes.c_double(0), ctypes.c_int(0)
        lib.ivosw_profile_stop(ctypes.byref(t2), ctypes.byref(c2))
        with open(args.layer_report, "w") as f:
            f.write(f"# per-layer conv timing (HIP events around every launch, 3 steps, batch {args.batch}, chunk {args.chunk or 'default'}, {args.precision})\n")
            f.write(buf.value.decode())
    outputs = {"scores": scores.float().cpu().numpy()} if args.dump_outputs else None
    if not args.full:
        return fps, dt, None, {}, outputs
    flops_step = GFLOP_PER_FRAME * 1e9 * args.batch
    achieved = flops_step / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    peak = {"bf16": PEAK_BF16_TFLOPS, "fp32": PEAK_F32_TFLOPS, "bf16x3": PEAK_BF16_TFLOPS / 3.0}[args.precision]
    # HBM bytes per launch of the same kernel family: from the committed rocprofv3 --pmc passes of this very command
    # (tools/profile_round.sh -> profiles/pmc_traffic_latest.json); only quoted when the launch count still matches
    traffic, traffic_src, hbm_gbps = None, None, None
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic_latest.json")
    if os.path.exists(tpath) and args.batch == 256 and args.precision == "bf16" and not args.chunk:
        tj = json.load(open(tpath))
        if abs(tj.get("launches_per_pass", -1) - launches) < 0.5:
            traffic, traffic_src = round(tj["bytes_per_launch"]), tj.get("source")
            hbm_gbps = round(tj["bytes_per_pass"] / (conv_ms * 1e-3) / 1e9, 1)
    dt_code = {"bf16": L.BF16, "fp32": L.F32, "bf16x3": L.F32X3}[args.precision]
    roof = {"bound": "mfma", "kernel": lib.ivosw_assess_dominant_kernel(dt_code).decode(), "achieved": round(achieved, 2),
            "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
            "hbm_GBps_of_family": hbm_gbps, "hbm_peak_GBps": 8000.0,
            "launches_per_step": launches, "avg_launch_us": round(conv_ms * 1e3 / max(launches, 1), 2),
            "flops_per_launch": flops_step / max(launches, 1), "kernel_ms_per_step": round(conv_ms, 3),
            "streams": 2 if split else 1,
            "reference_gemm": ({"tflops_8192_cubed": REFERENCE_GEMM_BF16_TFLOPS["gemm_8192"], "tflops_4096_cubed": REFERENCE_GEMM_BF16_TFLOPS["gemm_4096"],
                                "k_loop_tflops_at_tower_shapes": REFERENCE_GEMM_BF16_TFLOPS["k_loop_tower_shapes"],
                                "tower_over_reference_gemm": round(achieved / REFERENCE_GEMM_BF16_TFLOPS["gemm_8192"], 4),
                                "source": "committed reference measurement (profiles/r06_gemm_8phase_v1.txt, _v2.txt; one box, uniform random bf16), NOT re-measured in this run: "
                                          "the CDNA4 guide's plain-HIP 256x256 8-phase template as re-derived in ivos-w_amd/csrc/gemm_8phase.h; not a roof of the chip"}
                               if args.precision == "bf16" else None),
            "timing": "one HIP-event pair per forward pass around the tower's launches, inside the timed region (family time includes its own launch gaps)"
                      + ("; the batch runs as two halves on two streams: family time = latest end - earliest start of the halves' tower spans" if split else "")}
    if rank == 0 and args.precision == "bf16" and not args.no_clock_probe:
        # the clock / power the kernels ran at: frac stays against the 2.5 PFLOP/s of a 2.4 GHz chip;
        # frac_at_measured_clock is the same achieved rate against the MFMA peak AT THE MEASURED shader clock, beside it
        try:
            cp = measure_clock_and_power(step, dev, spin_us=max(500, int(dt / args.steps * 1e6 * 0.97)))
            roof.update(cp)
            if cp["sclk_mhz"] > 0:
                roof["peak_at_measured_clock"] = round(peak * cp["sclk_mhz"] / 2400.0, 1)
                roof["frac_at_measured_clock"] = round(achieved / (peak * cp["sclk_mhz"] / 2400.0), 4)
        except Exception as e:                            # a measurement aid must never cost the bench line
            roof["sclk_mhz"], roof["sclk_error"] = None, repr(e)[:160]
    extra = {"sustained": sus}
    if rank == 0:
        pick = [0, 37, 74, 111, 148, 185, 222, args.batch - 1] if args.batch >= 256 else list(range(min(8, args.batch)))
        extra["checked"] = True
        extra["check"] = check_scores(scores, tf, tp, args.precision, pick)
        extra["front"] = bench_front(args, dev, tf, tp)
        if args.precision == "bf16" and not args.no_fp32:
            extra["fp32"] = bench_fp32(args, dev, tf, tp, scores, pick)
            extra["bf16x3"] = bench_fp32(args, dev, tf, tp, scores, pick, precision="bf16x3")
    return fps, dt, roof, extra, outputs


def net_chunk(args):
    return args.chunk or (256 if args.precision == "bf16" else 64)      # the library defaults (assess.hip: default_chunk)


def bench_fp32(args, dev, tf, tp, scores16, pick, precision="fp32"):
    """The modes that meet north_star's 1e-4 on the same batch: "fp32" (exact fp32 MFMA: the parity gate) and "bf16x3" (fp32 tensors, every
    contraction, the stem included, as three bf16 MFMA passes on hi / lo splits, IVOSW_F32X3) — timed, checked against the oracle at 1e-4, and
    compared with the bf16 scores."""
    from ivos_w_amd.models.assessment import AssessNet
    net = AssessNet(precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net.to(dev).eval()
    out = {}

    def step():
        out["s"] = net(tf, tp)
    n = 4 if precision == "fp32" else 8
    dt = timed(step, n, 1, dev, None)
    s32 = out["s"].reshape(-1)
    rel = float(((scores16.reshape(-1) - s32).abs() / s32.abs()).max())
    if not (rel <= BF16_SCORE_RTOL):
        raise SystemExit(f"bench.py: bf16 scores differ from the {precision} mode by {rel:.3e} > {BF16_SCORE_RTOL}")
    chk = check_scores(s32, tf, tp, "fp32", pick)          # the 1e-4 bar for both
    fps = args.batch * n / dt
    tf_s = GFLOP_PER_FRAME * 1e9 * fps / 1e12
    peak = PEAK_F32_TFLOPS if precision == "fp32" else PEAK_BF16_TFLOPS / 3.0
    return {"value": round(fps, 1), "unit": "frames/s", "ms_per_step": round(dt / n * 1e3, 2), "steps": n, "dtype": "f32" if precision == "fp32" else "f32 tensors, 3 x bf16 MFMA",
            "achieved_TFLOPs": round(tf_s, 2), "peak_TFLOPs": round(peak, 1), "frac": round(tf_s / peak, 4),
            "note": ("whole-forward wall time (not kernel-only) against the fp32 MFMA peak" if precision == "fp32" else
                     "whole-forward wall time against a third of the bf16 MFMA peak (three passes per product); scores within 1e-4 of the oracle like the fp32 mode"),
            "bf16_vs_this_worst_rel": float(f"{rel:.3e}"), "check": chk}


def build_dqn(args, rank, dev):
    from ivos_w_amd.models.agent import Agent
    from ivos_w_amd.models.momory_pool import DeviceReplay
    agent = Agent(dev, agent_cfg())
    for net, seed in ((agent.policy_net, 0), (agent.target_net, 0)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(seed).items()})
    replay = DeviceReplay(synth.replay_transitions(n=args.replay, T=25, seed=2019), dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7 + 1000003 * rank)        # rank-offset minibatch stream
    np.random.seed(0)                          # target-sync coin: identical on every rank
    return agent, replay, gen


def bench_dqn(args, rank, world, dev, dist, steps, warmup):
    """One step = ONE hipGraphLaunch {minibatch draw (device-side counter-based generator) + replay gather, 3 forwards + loss + BPTT,
    [N=1: clamp + Adam with the device-side step]} -> [N>1: RCCL all-reduce of the 724 KB gradient arena, clamp + Adam] -> host coin -> target sync."""
    from ivos_w_amd.models.agent import CapturedDqnStep
    agent, replay, gen = build_dqn(args, rank, dev)
    B = args.minibatch
    from ivos_w_amd import parallel
    dp = world > 1 or args.dqn_dp_emulate or FORCE_DIST[0]     # the data-parallel step structure (gradients -> collective -> clamp + Adam)
    fused = not dp
    seed = 2019 + 7919 * rank
    lean = None
    if args.dqn_eager:
        cap = None
    elif dp and args.dqn_dp == "eager":
        # N > 1, default: plain launches (10 per step + the collective) from preallocated buffers.  A captured graph buys nothing
        # here — the host has a collective to enqueue every step anyway — and costs the 8.7 us bubble around each graph launch
        cap = None
        lean = dict(draw=replay.draw_state(seed), bufs=None)
    else:
        cap = CapturedDqnStep(agent, replay, B, fused=fused, draw_seed=None if os.environ.get("IVOSW_BENCH_HOST_DRAW") else seed)
    nrep = len(replay)
    # N > 1: the step is timed through the backend's collective: torch.distributed's all-reduce (RCCL over xGMI; gloo staged through the
    # host in the one-GPU tests) followed by the fused clamp + Adam kernel.  That is the product default and it is dqn.value.
    # The one-shot peer-to-peer all-reduce fused with clamp + Adam (two launches; opt-in in the product, IVOSW_P2P=1) is attempted by
    # DEFAULT too (an 8-GPU node may run this build exactly once, and that one run has to answer both questions),
    # but as the LAST thing main() does, after every other number of the line exists (info["_p2p_leg"] below): its cross-GPU path
    # (IPC-mapped peer arenas, system-scope flags) has only ever run between two processes on ONE device.  The set-up is collective
    # and self-tested against the backend's result, a peer timeout raises on every rank, every failure lands in
    # dqn.collectives.p2p.error, and a process that DIES in that leg still leaves the line behind (LineGuard).  IVOSW_BENCH_P2P=0
    # (or IVOSW_P2P=0) skips the leg.
    legs = ["backend"] if (FORCE_DIST[0] or world > 1) else [None]
    want_p2p = args.full and world > 1 and os.environ.get("IVOSW_BENCH_P2P", "1") != "0" and os.environ.get("IVOSW_P2P", "") != "0" and dev.type == "cuda"

    def select_leg(name):
        if name is None:
            return None
        os.environ["IVOSW_P2P"] = "1" if name == "p2p" else "0"
        for v in parallel._P2P.values():
            if v is not None:
                v.close()
        parallel._P2P.clear()
        return parallel.p2p_for(agent.policy_net.flat_grad)       # collective decision (self-test), outside the timed region

    def step():
        if lean is not None:
            lean["bufs"] = replay.sample_drawn(B, lean["draw"], out=lean["bufs"])
            agent.loss_and_grads(lean["bufs"])
        elif cap is None:
            idx = torch.randint(0, nrep, (B,), device=dev, generator=gen)
            agent.loss_and_grads(replay.sample(idx))
        else:
            if cap.draw is None:                # (IVOSW_BENCH_HOST_DRAW=1: the minibatch rows from torch's generator, one more launch)
                torch.randint(0, nrep, (B,), device=dev, generator=gen, out=cap.idx)
            cap.launch()
        if cap is None or not fused:
            agent.apply_gradients(check_every=8)        # N > 1: all-reduce (selected path) + clamp + Adam; N = 1: clamp + Adam
        if np.random.random() < agent.update_rate:
            agent.sync_target()
    loop, launch_mode = None, None
    leg_us = {}
    if cap is not None and fused and cap.draw is not None and args.dqn_block > 1:
        # N = 1: the same steps in blocks of `dqn_block` per hipGraphLaunch whenever no target-sync coin of the block fires
        # (GraphedDqnLoop: same coin stream, same minibatch stream, bit-identical results; an 8.7 us bubble separates two
        # graph launches).  Timed like `timed()`: warm-up, synchronize, EXACTLY `steps` steps, synchronize.
        # Launch mode (--dqn-mode): "graph" = those blocks, "plain" = ten plain launches per step from preallocated buffers (no
        # bubble between graph launches; needs a host that keeps ahead of ~190 us of GPU work per step), "auto" (default) = the
        # warm-up runs 2 x 128 steps through each and the timed region uses the faster one.  The modes are bit-identical.
        from ivos_w_amd.models.agent import AutoDqnLoop
        auto = AutoDqnLoop(agent, replay, B, draw_seed=2019 + 7919 * rank, block=args.dqn_block)
        if args.dqn_mode != "auto":
            auto.choice = args.dqn_mode
        cap = auto.graphed.one
        t_w = time.perf_counter()
        auto.run(max(warmup, 2 * auto.probe if auto.choice is None else 0))
        torch.cuda.synchronize(dev)
        while time.perf_counter() - t_w < min(args.min_warm_s, 0.5):
            auto.run(max(1, warmup))
            torch.cuda.synchronize(dev)
        loop = auto.graphed if auto.choice == "graph" else None
        l0 = auto.graphed.launches
        t0 = time.perf_counter()
        auto.run(steps)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        launches_per_step = (auto.graphed.launches - l0) / steps if auto.choice == "graph" else 8.0
        launch_mode = {"mode": auto.choice, "requested": args.dqn_mode, "probe_us_per_step": {k: round(v, 1) for k, v in auto.probe_us.items()}}
    else:
        dt = None
        for leg in legs:
            select_leg(leg)
            dt = timed(step, steps, warmup, dev, dist, min(args.min_warm_s, 0.5))
            if leg is not None:           # what actually carried the gradients: the process group's own answers, not this script's flags
                leg_us[leg] = {"us_per_step": round(dt / steps * 1e6, 1), "steps_per_sec_all_ranks": round(world * steps / dt, 1), "steps": steps,
                               "world_size": int(dist.get_world_size()), "backend": str(dist.get_backend())}

    def p2p_leg():
        """The guarded late leg (collective: every rank calls it).  Returns the dqn.collectives.p2p record."""
        n_leg = min(steps, 500)
        try:
            h = select_leg("p2p")
        except Exception as e:                          # the set-up is collective; a failure here is the same on every rank
            return {"error": repr(e)[:200]}
        if h is None:
            return {"skipped": "the self-test did not pass on every rank (or fine-grained / IPC memory is unavailable)"}
        # a path that has never run across GPUs: short timeout, frequent error checks, fewer steps; a peer timeout raises on every rank
        # within a few steps (the ranks that did arrive time out on the missing one) and the barrier re-aligns them
        h.timeout_ms = 250
        try:
            d = timed(step, n_leg, warmup, dev, dist, min(args.min_warm_s, 0.5))
            torch.cuda.synchronize(dev)
            if h.error() != 0:
                raise RuntimeError("the peer-to-peer all-reduce timed out waiting for a rank")
        except RuntimeError as e:
            torch.cuda.synchronize(dev)
            dist.barrier()
            return {"error": str(e)[:200]}
        finally:
            os.environ["IVOSW_P2P"] = "0"
        us = d / n_leg * 1e6
        return {"us_per_step": round(us, 1), "steps_per_sec_all_ranks": round(world * n_leg / d, 1), "steps": n_leg,
                "path": "one-shot xGMI peer-to-peer all-reduce fused with clamp + Adam (ivosw_p2p_allreduce_clamp_adam, self-tested against the backend's result at start-up)",
                "vs_backend": round(leg_us["backend"]["us_per_step"] / us, 3),
                "scaling_vs_1gpu": round(world * n_leg / d / DQN_1GPU_REF["steps_per_sec"], 3)}
    assert torch.isfinite(agent.policy_net.flat).all() and agent.optimizer.state["step"] >= steps + warmup
    # what the timed steps left behind, before anything below trains the same agent further (--dump-outputs)
    outputs = ({"policy_params": agent.policy_net.flat.cpu().numpy(), "target_params": agent.target_net.flat.cpu().numpy()}
               if args.dump_outputs else None)
    sps = world * steps / dt
    per_gpu_tflops = DQN_GFLOP_PER_STEP * 1e9 * (sps / world) / 1e12
    info = {"us_per_step": round(dt / steps * 1e6, 1), "graph": (cap is not None) if launch_mode is None else launch_mode["mode"] == "graph",
            # whole-job DQN steps/s over the committed single-GPU rate (weak scaling: minibatch 128 per GPU); north_star asks >= 6 at N = 8
            "scaling_vs_1gpu": {"value": round(sps / DQN_1GPU_REF["steps_per_sec"], 3), "n_gpus": world, "reference": DQN_1GPU_REF} if world > 1 or FORCE_DIST[0] else None,
            "launch_mode": launch_mode, "_outputs": outputs,
            "step_structure": "data-parallel: gradients -> collective -> clamp + Adam" + (" (emulated at N = 1, no collective)" if world == 1 and not FORCE_DIST[0] else " (forced at N = 1: the collective runs over one rank)" if world == 1 else "") if dp else "single GPU: fused step",
            "collective_path": (("RCCL all-reduce" if BACKEND[0] == "nccl" else "gloo all-reduce staged through host memory") if world > 1 or FORCE_DIST[0] else None),
            "collectives": (leg_us if (world > 1 or FORCE_DIST[0]) and launch_mode is None else None),
            "_p2p_leg": p2p_leg if want_p2p and launch_mode is None else None,        # run by main() as its last act; never serialised
            "kernel_nodes_in_graph": cap.kernel_nodes if cap is not None else None,
            "host_launches_per_step": (round(launches_per_step, 3) if launch_mode is not None else (1 if fused else 3) + (cap.draw is None)) if cap is not None else None,
            "steps_per_graph_launch": args.dqn_block if loop is not None else (1 if cap is not None else None),
            "minibatch_draw": "device (ivosw_replay_draw_gather, inside the graph)" if cap is not None and cap.draw is not None else "torch.randint",
            "roofline": {"bound": "mfma", "achieved": round(per_gpu_tflops, 3), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(per_gpu_tflops / PEAK_F32_TFLOPS, 5), "traffic": None,
                         "note": "whole step (10.5 GFLOP algorithmic, SURVEY 8d) / step wall time per GPU, against the fp32 MFMA peak: the step is a "
                                 "chain of dependent launches (latency-bound), so this fraction is reported for completeness"}}
    # The API the reference's loop actually calls: utils_agent.agent_business -> up to 14 x
    # Agent.update_agent(sample) per episode on COLLATED HOST batches of the replay dataset through a shuffling DataLoader
    # (train_agent.py:175-182, utils/utils_agent.py:244-252), the loss returned as a float every step — and the device loop
    # agent_business takes instead when the loader is this build's own dataset (same minibatches, bit-identical results).
    if args.full and rank == 0 and world == 1:
        from torch.utils.data import DataLoader
        from ivos_w_amd.datasets.agent_dataset import DAVIS2017AgentTrain
        from ivos_w_amd.utils import utils_agent
        import contextlib
        import io
        ds = DAVIS2017AgentTrain.from_soa(synth.replay_transitions(n=min(args.replay, 20000), T=25, seed=2019))
        api = {}
        for name in ("update_agent_per_collated_batch", "agent_business_device_loop"):
            os.environ["IVOSW_UPDATE_PATH"] = "host" if name.startswith("update_agent") else ""
            episodes, n_steps = 12, 0
            with contextlib.redirect_stdout(io.StringIO()):
                for ep in range(episodes + 2):
                    if ep == 2:
                        torch.cuda.synchronize(dev)
                        t0, n_steps = time.perf_counter(), 0
                    loader = DataLoader(ds, batch_size=B, shuffle=True, num_workers=0)
                    got = utils_agent._device_update_loop(agent, loader, 14)
                    if got is None:
                        got = []
                        for i, sample in enumerate(loader):
                            if i == 14:
                                break
                            got.append(agent.update_agent(sample))
                    n_steps += len(got)
            torch.cuda.synchronize(dev)
            dt_api = time.perf_counter() - t0
            api[name] = {"steps_per_sec": round(n_steps / dt_api, 1), "us_per_step": round(dt_api / n_steps * 1e6, 1)}
        os.environ.pop("IVOSW_UPDATE_PATH", None)
        api["note"] = ("12 episodes x 14 steps, minibatch %d, DataLoader(shuffle=True) over %d transitions, loader construction and shuffle "
                       "included; the per-batch path pays the DataLoader collation (128 dict samples -> 8 tensors), eight H2D copies and a "
                       "loss.item() per step" % (B, len(ds)))
        info["update_agent_api"] = api
    # Agent.action latency at evaluation size (N = 1, T = 104 frames: host state -> greedy index on the host)
    if args.full and rank == 0:
        state = synth.brain_inputs(1, 104, 3)[0]
        agent.cfg = AD(agent.cfg, phase="eval")
        for _ in range(5):
            agent.action(state, verbose=False)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(50):
            agent.action(state, verbose=False)
        info["action_latency_us_T104"] = round((time.perf_counter() - t0) / 50 * 1e6, 1)
    return sps, dt, info


def bench_jf(rank, world, dev, dist, steps=20, warmup=3, N=100, O=3):
    """DAVIS J and F of one 100-frame 480p sequence with 3 objects per step, label maps resident in
    HBM as uint8, counts left on the device (the host ratio step is a few hundred float64 divisions).  HBM-bound:
    algorithmic bytes = 2 label maps read once."""
    from ivos_w_amd import metrics
    gt, pr = synth.label_maps(N, 480, 854, O, seed=4 + rank)
    tg, tp = torch.from_numpy(gt).to(dev), torch.from_numpy(pr).to(dev)
    lib = L.lib()
    counts = torch.empty((N, O, 6), dtype=torch.int64, device=dev)
    nbytes = lib.ivosw_jf_ws_bytes(N, 480, 854, O)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ids = bytes(range(1, O + 1))
    st = L.stream_ptr(dev)

    def step():
        L.check(lib.ivosw_jf_counts(L.dptr(tg), L.dptr(tp), N, 480, 854, ids, O, 8, L.dptr(counts), L.dptr(ws), nbytes, st), "jf")
    dt = timed(step, steps, warmup, dev, dist)
    fps = world * N * steps / dt
    out = {"metric": "jf_scored_frames_per_sec", "value": round(fps, 1), "unit": "frames/s (480p, 3 objects, J and F)",
           "us_per_sequence": round(dt / steps * 1e6, 1), "dtype": "u8",
           "roofline": {"bound": "hbm", "achieved": round(2 * N * 480 * 854 * steps / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(2 * N * 480 * 854 * steps / dt / 8e12, 4),
                        "note": "algorithmic bytes = both label maps read once (820 KB per frame); the boundary-match pass works on bit maps 8x smaller"}}
    if rank == 0 and world == 1:
        from oracle import jf_oracle as jo          # checker + CPU baseline only
        j, f = metrics.batched_j_and_f(tg[:4], tp[:4], nb_objects=O)
        assert np.array_equal(j, jo.batched_jaccard(gt[:4], pr[:4], nb_objects=O)) and np.array_equal(f, jo.batched_f_measure(gt[:4], pr[:4], nb_objects=O))
        t0 = time.perf_counter()
        jo.sequence_metric("J_AND_F", gt[:8], pr[:8], O)
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(8 / cdt, 2), "unit": "frames/s", "cores": 1, "kind": "port",
                               "sample": "8 frames x 3 objects, numpy/scipy oracle of davisinteractive's batched_jaccard + batched_f_measure"}
    return out


def bench_seg(rank, world, dev, dist, steps=20, warmup=3, n=100, C=4):
    """upsample + argmax + softmax epilogue for one 100-frame sequence per step (stride-4 logits of
    3 objects + background -> 480p), probabilities written once, object-major.  HBM-bound on the outputs."""
    from ivos_w_amd.utils import utils_manet
    g = torch.Generator(device=dev).manual_seed(5 + rank)
    x = torch.randn(n, C, 120, 214, device=dev, generator=g) * 3
    store = utils_manet.ProbStore(n, C, 480, 854, dev)

    def step():
        utils_manet.seg_epilogue(x, 480, 854, store, 0)
    dt = timed(step, steps, warmup, dev, dist)
    out_bytes = n * 480 * 854 * (C * 4 + 8 + 1 + 4)       # probs + int64 / uint8 / float labels
    res = {"metric": "seg_epilogue_frames_per_sec", "value": round(world * n * steps / dt, 1), "unit": "frames/s (480p, 4 channels)",
           "us_per_sequence": round(dt / steps * 1e6, 1), "dtype": "f32",
           "roofline": {"bound": "hbm", "achieved": round(out_bytes * steps / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(out_bytes * steps / dt / 8e12, 4),
                        "note": "algorithmic bytes = outputs written once (29 B per pixel); the stride-4 logits are 1/16 of a channel plane"}}
    if rank == 0 and world == 1:
        from oracle import seg_oracle as so           # checker + CPU baseline only
        xc = x[:4].cpu()
        t0 = time.perf_counter()
        up, lab = so.epilogue(xc, 480, 854)
        pc = torch.softmax(up, 1)
        cdt = time.perf_counter() - t0
        assert (store.all_P[:4].cpu() - pc).abs().max().item() < 2e-6
        res["cpu_baseline"] = {"value": round(4 / cdt, 2), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": "4 frames, torch-CPU interpolate + argmax + softmax (the reference's own calls)"}
    return res


def bench_recommend(rank, dev, n=100, O=3, reps=8):
    """one frame recommendation of the interaction loop (utils/utils_agent.py:104-122, wild / ours) on a
    100-frame 480p sequence with 3 objects — all_F arrives as the HOST tensor the entry scripts hold, all_P is on the device.
    Product path: the video is uploaded once per sequence and cached, all objects are scored in one pass over one copy of the
    frames, quality -> state -> Brain -> argmax stays on the device.  Beside it the reference's data movement on the same
    kernels: upload all_F every interaction, one AssessNet forward per object, numpy mean, host-side action()."""
    from ivos_w_amd.models.agent import Agent
    from ivos_w_amd.models.assessment import AssessNet
    from ivos_w_amd.utils import utils_agent
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net.to(dev).eval()
    agent = Agent(dev, AD(agent_cfg(), phase="eval"))
    g = torch.Generator().manual_seed(11)
    all_F = torch.rand(n, 3, 480, 854, generator=g)
    logits = torch.randn(n, O + 1, 120, 214, generator=g) * 3
    all_P = torch.softmax(torch.nn.functional.interpolate(logits.to(dev), (480, 854), mode="bilinear", align_corners=True), 1).contiguous()
    quality = np.zeros(n)
    kw = dict(n_frame=n, n_objects=O, all_F=all_F, all_P=all_P, new_masks_quality=np.zeros(n), prev_frames=[5], annotated_frames_list=[5],
              mask_quality=quality, first_frame=5, max_nb_interactions=8)
    cfg = AD(setting="wild", method="ours")
    utils_agent.clear_frame_cache()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    first = int(utils_agent.recommend_frame(cfg, net, agent, dev, **kw))
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(reps):
        nxt = int(utils_agent.recommend_frame(cfg, net, agent, dev, **kw))
    t_next = (time.perf_counter() - t0) / reps
    assert nxt == first

    def reference_flow():
        fdev = all_F.to(dev)
        pred = np.zeros((n, O))
        for i in range(O):
            pred[:, i] = net(fdev, all_P[:, i + 1].contiguous()).cpu().numpy().reshape(-1)
        q = pred.mean(1)
        counts = np.zeros(n)
        counts[5] += 1
        return int(agent.action(np.stack([q, counts], 1), verbose=False))
    ref_pick = reference_flow()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(3):
        reference_flow()
    t_ref = (time.perf_counter() - t0) / 3
    assert ref_pick == first, (ref_pick, first)
    # evaluation-size launches: what recommend_frame issues per interaction is ONE forward over frames x objects units
    # (utils/utils_agent.py:111-122), 50 - 300 units, not the 256-frame headline batch.  Whole-forward wall time (front end included)
    # by HIP events, video and masks resident; frac = units x 10.779 GFLOP / time / 2.5 PFLOP/s.
    eval_sizes = {}
    fdev = all_F.to(dev)
    for nf, no in ((100, 1), (100, 3), (70, 2)):
        Fv, Pv = fdev[:nf].contiguous(), all_P[:nf, :no + 1].contiguous()
        for _ in range(6):
            net.forward_objects(Fv, Pv, no)
        reps_e = 30
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(reps_e):
            net.forward_objects(Fv, Pv, no)
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / reps_e
        units = nf * no
        eval_sizes[f"{nf}x{no}"] = {"units": units, "ms": round(ms, 3), "units_per_s": round(units / ms * 1e3, 1),
                                    "frac": round(units * GFLOP_PER_FRAME / ms / PEAK_BF16_TFLOPS, 4)}
    return {"metric": "recommend_frame_latency_ms", "frames": n, "objects": O, "first_call_ms": round(t_first * 1e3, 2),
            "eval_sizes": eval_sizes,
            "value": round(t_next * 1e3, 2), "unit": "ms per interaction (video cached on the device)",
            "reference_data_movement_ms": round(t_ref * 1e3, 2),
            "note": "same kernels both ways; the reference re-uploads the 492 MB video and runs one forward per object every interaction (utils/utils_agent.py:114-119)",
            "same_recommendation": True}


def cpu_baseline_assess():
    """The oracle (torch-CPU restatement of AssessNet.forward) on BASELINE configs[0] (8 synthetic 480p pairs), timed at several thread
    counts: oneDNN convolutions at 8 x 256^2 stop scaling well before the host's core count, so the sweep and every value are in the
    record and `value` / `cores` are the best of them."""
    from oracle import assess_oracle as ao
    sd = ao.to_torch_sd(synth.assessnet_state_dict(0))
    tf, tp = synth.assess_inputs(8, seed=1234)
    ncpu = os.cpu_count() or 1
    tried = {}
    for threads in sorted({min(8, ncpu), min(16, ncpu), min(32, ncpu), min(64, ncpu)}):
        torch.set_num_threads(threads)
        ao.assess_forward(sd, tf, tp)
        reps, t0 = 0, time.perf_counter()
        while reps < 2 or (time.perf_counter() - t0 < 4.5 and reps < 40):
            ao.assess_forward(sd, tf, tp)
            reps += 1
        tried[threads] = (8 * reps / (time.perf_counter() - t0), reps)
    best = max(tried, key=lambda k: tried[k][0])
    torch.set_num_threads(best)
    return {"value": round(tried[best][0], 2), "unit": "frames/s", "cores": best, "host_cores": ncpu, "kind": "port",
            "threads_tried": {str(k): round(v[0], 2) for k, v in tried.items()},
            "sample": f"{tried[best][1]} x AssessNet.forward on 8 synthetic 480p pairs (BASELINE configs[0]) per thread count, torch-CPU oracle; best of the sweep"}


def cpu_baseline_dqn():
    """the stock torch-CPU path (nn.Linear / nn.LSTMCell / autograd / optim.Adam assembled by own module definitions,
    pinned against the reference's goldens in tests/test_oracle_brain.py) on the host cores."""
    from oracle.torch_cpu_baseline import TorchDQN
    tr = synth.replay_transitions(n=2000, T=25, seed=2019)
    best = None
    for threads in sorted({min(8, os.cpu_count() or 1), min(16, os.cpu_count() or 1), min(32, os.cpu_count() or 1)}):
        # the step is ~1000 tiny ops: it stops scaling after a few threads (and crawls at 256), so 8 / 16 / 32 are tried and the best is reported
        torch.set_num_threads(threads)
        dqn = TorchDQN(synth.brain_state_dict(0), synth.brain_state_dict(0))
        rs = np.random.RandomState(0)
        reps, t0 = 0, time.perf_counter()
        while reps < 3 or (time.perf_counter() - t0 < 4.0 and reps < 200):
            batch = synth.collate_np(tr, synth.minibatch_indices(reps % 8, n=2000, B=128, seed=7))
            dqn.update(batch, rs.random_sample())
            reps += 1
        v = reps / (time.perf_counter() - t0)
        if best is None or v > best[0]:
            best = (v, threads, reps)
    return {"value": round(best[0], 2), "unit": "steps/s", "cores": best[1], "host_cores": os.cpu_count(), "kind": "port",
            "sample": f"{best[2]} x update_agent, minibatch 128, T=25, torch-CPU (LSTMCell / autograd / Adam, the reference's operator sequence); "
                      f"best of several thread counts"}


class LineGuard:
    """Keeps the JSON line alive across a leg that may take the process down.  A child process holds the finished line (with
    collectives.p2p = the failure note) and the read end of a pipe; it prints the line to the inherited stdout iff the pipe closes
    without the one byte disarm() sends.  Works for any death of the parent (abort() inside the HIP runtime, SIGKILL from the launcher)."""
    CHILD = ("import sys,os\n"
             "fd=int(sys.argv[1]); line=sys.stdin.buffer.read(); sys.stdin.close()\n"
             "b=os.read(fd,1)\n"
             "if not b: sys.stdout.buffer.write(line+b'\\n'); sys.stdout.flush()\n")

    def __init__(self, line, rec):
        import subprocess
        saved = rec.get("p2p")
        rec["p2p"] = {"error": "the process died inside the peer-to-peer leg (hard fault); every other number of this line was measured before it started; "
                               "line printed by the watchdog child"}
        payload = json.dumps(line).encode()
        if saved is None:
            rec.pop("p2p")
        else:
            rec["p2p"] = saved
        r, self.w = os.pipe()
        self.child = subprocess.Popen([sys.executable, "-c", self.CHILD, str(r)], stdin=subprocess.PIPE, pass_fds=(r,), close_fds=True)
        os.close(r)
        self.child.stdin.write(payload)
        self.child.stdin.close()

    def disarm(self):
        try:                                   # (a child that is already gone cannot print either: nothing to do)
            os.write(self.w, b"k")
            os.close(self.w)
            self.child.wait(timeout=10)
        except Exception:
            pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--min-warm-s", type=float, default=1.0, help="extend the warm-up to at least this many seconds (steady-state clocks)")
    ap.add_argument("--no-fp32", action="store_true", help="skip the fp32 parity-mode sub-record")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl", help="torch.distributed backend for --gpus > 1 (nccl = RCCL)")
    ap.add_argument("--dqn-eager", action="store_true", help="DQN leg with eager launches instead of the captured HIP graph")
    ap.add_argument("--workload", choices=["assess", "dqn"], default="assess")
    ap.add_argument("--batch", type=int, default=256, help="frames per GPU per step (assessment); with --scaling strong: frames per step of the whole job")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default): --batch frames per GPU; strong: --batch frames in total, sharded contiguously over the ranks (SURVEY 8e: 256 total)")
    ap.add_argument("--precision", choices=["bf16", "fp32", "bf16x3"], default="bf16")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--minibatch", type=int, default=128)
    ap.add_argument("--replay", type=int, default=50000)
    ap.add_argument("--dqn-steps", type=int, default=2000)
    ap.add_argument("--dqn-mode", choices=["auto", "graph", "plain"], default="auto", help="N = 1: how the training steps are launched (auto: measured in the warm-up)")
    ap.add_argument("--dqn-dp", choices=["eager", "graph"], default="eager", help="N > 1: plain launches (default) or a captured graph for the gradient part of the step")
    ap.add_argument("--dqn-dp-emulate", action="store_true", help="N = 1: run the data-parallel step structure (no collective) to time it")
    ap.add_argument("--dqn-block", type=int, default=8, help="N = 1: training steps per hipGraphLaunch when no target-sync coin of the block fires (1 = one graph launch per step)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-dist", action="store_true", help="N = 1 through the N > 1 branch: a process group of one rank on the chosen backend, barrier + "
                    "max over ranks around the timed region, the gradient all-reduce in every DQN step (RCCL on a one-GPU box)")
    ap.add_argument("--no-dp-critical-path", action="store_true", help="skip the child run that times the DQN step through the collective branch at world size 1")
    ap.add_argument("--layer-report", default="", help="write a per-conv-layer timing table (HIP events) to this file")
    ap.add_argument("--no-clock-probe", action="store_true", help="skip the 15 extra forward passes that measure roofline.sclk_mhz / power_w (profiling runs count passes)")
    ap.add_argument("--no-live-traffic", action="store_true", help="do not re-run the forward under rocprofv3 --pmc for roofline.traffic (the committed PMC summary is quoted instead)")
    ap.add_argument("--tower-only", action="store_true", help="(internal: the rocprofv3 --pmc sub-runs) build the inputs, run warmup + steps forward passes, print nothing else")
    ap.add_argument("--full", action="store_true", help="measure and check everything beyond the headline figure: oracle check, roofline (span timing, "
                    "clock / power probe, PMC traffic), sustained rate, DQN leg, fp32 / bf16x3 modes, front end, recommend_frame, J&F, seg epilogue, "
                    "CPU baselines, the DQN data-parallel and P2P legs.  Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the timed path returned in its last step "
                    "as DIR/<name>.npy (float32): `scores` of the assessment workload, `policy_params` / `target_params` of the DQN workload")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # a plain `python bench.py --gpus N`: become the launcher — one rank per GPU under torch.distributed.run, exactly the
        # command the driver uses (rendezvous on 127.0.0.1: the container hostname may not resolve); rank 0 prints the line.
        # The launcher is a child process and this one never touches the GPU
        import subprocess
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:], env=env)
        raise SystemExit(r.returncode)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: there is no CPU fallback for the hot path")
    BACKEND[0] = args.backend
    if args.force_dist:
        if args.gpus != 1:
            raise SystemExit("--force-dist is the N = 1 run through the N > 1 branch")
        FORCE_DIST[0] = True
        os.environ["IVOSW_FORCE_DIST"] = "1"            # parallel.data_parallel_step: the collective runs over the one rank
    rank, world, dev, dist = dist_setup(args.gpus)
    args.total_batch = args.batch * world
    if args.scaling == "strong" and world > 1:
        from ivos_w_amd import parallel as _par
        args.total_batch = args.batch
        lo, hi = _par.shard_range(args.batch, rank, world)         # contiguous, balanced shards of the fixed total (no data-path collective)
        args.batch = hi - lo
        assert args.batch > 0, "strong scaling needs at least one frame per rank"
    lib = L.lib()
    # ablation guard: the measured library must be the default build, with no debug switch in the environment
    if lib.ivosw_ablation_build() != 0 or os.environ.get("IVOSW_DEBUG_CONV", "0") not in ("", "0") or os.environ.get("IVOSW_TUNE_BDBG", "0") not in ("", "0"):
        raise SystemExit("bench.py: ablation switches are compiled in or set (IVOSW_ABLATION build / IVOSW_DEBUG_CONV / IVOSW_TUNE_BDBG): refusing to measure")

    if args.tower_only:
        net, tf, tp = build_assess(args, rank, dev)
        for _ in range(args.warmup + args.steps):
            net(tf, tp)
        torch.cuda.synchronize(dev)
        print(json.dumps({"tower_only_passes": args.warmup + args.steps}), flush=True)
        return
    line = {"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "data": "synthetic"}
    if FORCE_DIST[0]:
        line["force_dist"] = f"process group of one rank on {BACKEND[0]}: barrier + max over ranks around every timed region, all-reduce in every DQN step"
    if args.workload == "assess":
        fps, dt, roof, extra, outputs = bench_assess(args, rank, world, dev, dist)
        line.update({"metric": "assessed_frames_per_sec", "value": round(fps, 1), "unit": "frames/s",
                     "ms_per_step": round(dt / args.steps * 1e3, 3), "dtype": args.precision,
                     "config": {"workload": (f"AssessNet.forward, batch {args.batch} x 480x854 frame+mask per GPU (BASELINE configs[1])" if args.scaling == "weak" or world == 1 else
                                             f"AssessNet.forward, batch {args.total_batch} x 480x854 frame+mask in total, sharded over the ranks (BASELINE configs[1], strong scaling)"),
                                "batch_per_gpu": args.batch, "total_batch": args.total_batch, "chunk": args.chunk or "default", "parallelism": f"frames sharded x{world}"},
                     "ablation_build": 0})
        if args.full:
            if rank == 0 and world == 1 and not args.no_live_traffic and args.batch == 256 and args.precision == "bf16" and not args.chunk:
                live = live_traffic(roof["kernel"], roof["launches_per_step"], roof["kernel_ms_per_step"])
                if live is not None:
                    roof.update(live)
            dqn_sps, dqn_dt, dqn_info = bench_dqn(args, rank, world, dev, dist, args.dqn_steps, 20)
            dqn_info.pop("_outputs")
            late_p2p = dqn_info.pop("_p2p_leg")
            line.update({"roofline": roof,
                         "dqn": dict({"metric": "dqn_agent_steps_per_sec", "value": round(dqn_sps, 1), "unit": "minibatch-steps/s (all ranks)",
                                      "transitions_per_sec": round(dqn_sps * args.minibatch, 1), "minibatch_per_gpu": args.minibatch,
                                      "replay": args.replay, "T": 25, "steps": args.dqn_steps,
                                      "dtype": "f32", "collective": (dqn_info.get("collective_path") + " (724 KB)") if world > 1 or FORCE_DIST[0] else None}, **dqn_info)})
            line.update(extra)
    else:
        sps, dt, info = bench_dqn(args, rank, world, dev, dist, args.steps, args.warmup)
        roof = info.pop("roofline")
        outputs = info.pop("_outputs")
        late_p2p = info.pop("_p2p_leg")
        line.update({"metric": "dqn_agent_steps_per_sec", "value": round(sps, 1), "unit": "minibatch-steps/s",
                     "ms_per_step": round(dt / args.steps * 1e3, 4), "dtype": "f32",
                     "config": {"workload": f"Double-DQN update, replay {args.replay}, minibatch {args.minibatch}/GPU, T=25 (BASELINE configs[2]/[3])",
                                "parallelism": f"dp{world}"},
                     "roofline": roof, "ablation_build": 0}, **info)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, outputs, rank, world)
    if args.full:
        if args.workload == "assess":
            if rank == 0 and world == 1 and not args.no_cpu_baseline:
                line["recommend_frame"] = bench_recommend(rank, dev)
            line["jf"] = bench_jf(rank, world, dev, dist)
            line["seg_epilogue"] = bench_seg(rank, world, dev, dist)
            if args.no_cpu_baseline:
                line["jf"].pop("cpu_baseline", None)
                line["seg_epilogue"].pop("cpu_baseline", None)
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline_assess() if args.workload == "assess" else cpu_baseline_dqn()
            if args.workload == "assess":
                line["dqn"]["cpu_baseline"] = cpu_baseline_dqn()
                if not FORCE_DIST[0] and not args.no_dp_critical_path:
                    line["dqn"]["dp_critical_path"] = dqn_dp_critical_path(line["dqn"]["us_per_step"])
                if not args.no_live_traffic:
                    dt_live = dqn_live_traffic()
                    if dt_live is not None:
                        line["dqn"]["roofline"].update(dt_live)
        if late_p2p is not None:
            # every other number of the line exists now.  Rank 0 hands the line to a watchdog child before the leg starts: if this process
            # dies in it (a GPU fault aborts the process from inside the HIP runtime, where no Python handler runs), the child prints the
            # line with the failure recorded; otherwise the leg's record goes into the line and this process prints it as usual.
            rec = (line["dqn"] if args.workload == "assess" else line)["collectives"]
            try:
                guard = LineGuard(line, rec) if rank == 0 else None
            except Exception:                      # no watchdog (fork refused, ...): the leg still runs, the line is printed below as always
                guard = None
            rec["p2p"] = late_p2p()
            if guard is not None:
                guard.disarm()
    if rank == 0:
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
