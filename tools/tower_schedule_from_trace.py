"""Tower launches of ONE ivosw_assess_forward out of a `rocprofv3 --kernel-trace --output-format csv` file, as the text that
tests/golden/tower_schedule/ keeps: per stream, in enqueue order, "stream kernel workgroups workgroup_size" with the kernel name cut at '<'.
Everything that is not a tower kernel (weight packing, mask box, ROI sampler, pool + fc, runtime copy kernels) is dropped.

usage: tower_schedule_from_trace.py KERNEL_TRACE.csv "precision=bf16 B=8 chunk=0 tap_stage=0" ["KEY=VAL ..."] > golden.txt"""
import csv
import re
import subprocess
import sys

TOWER = {"conv_igemm_kernel", "conv_igemm_dma_kernel", "conv_igemm_ws_kernel", "conv3x3_patch_kernel", "conv3x3_patch_x3_kernel", "conv1x1_wide_kernel",
         "gemm_8phase_kernel", "stem_pool_kernel", "stem_pool_x3_kernel", "maxpool_kernel", "maxpool_x3_kernel", "res2_chain_kernel", "res2_stage_kernel",
         "stage_first_kernel", "bneck64_kernel", "bneck_halo_kernel", "bneck_halo64s_kernel", "bneck_halo128s_kernel", "bneck_half16_kernel",
         "bneck_wide_kernel", "bneck_wide_stage_kernel", "res2_tail_x3_kernel", "res3_tail_x3_kernel"}


def short(name):
    if name.endswith(".kd"):
        name = name[:-3]
    if name.startswith("_Z"):
        name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    name = re.split(r"[<(]", name, 1)[0].strip()
    return name.split()[-1].split("::")[-1]


def schedule(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    key = "Stream_Id" if "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows}) > 1 else "Queue_Id"
    streams, out = [], {}
    for r in rows:
        k = short(r["Kernel_Name"])
        if k not in TOWER:
            continue
        if r[key] not in streams:
            streams.append(r[key])
        wg = int(r["Workgroup_Size_X"]) * int(r.get("Workgroup_Size_Y", 1) or 1) * int(r.get("Workgroup_Size_Z", 1) or 1)
        grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)
        out.setdefault(streams.index(r[key]), []).append((k, grid // wg, wg))
    return [(s, *t) for s in sorted(out) for t in out[s]]


if __name__ == "__main__":
    print("# tower launches of one ivosw_assess_forward: kernel trace of the commit before the schedule refactor (tools/tower_schedule_from_trace.py)")
    print("# config: " + sys.argv[2])
    if len(sys.argv) > 3 and sys.argv[3].strip():
        print("# tune: " + sys.argv[3])
    print("# stream kernel workgroups workgroup_size")
    for row in schedule(sys.argv[1]):
        print(*row)
