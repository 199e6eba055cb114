"""The tower's schedule as data: ivosw_assess_describe (no device) against kernel traces of the commit before the schedule refactor,
and against what a forward pass really enqueues.

tests/golden/tower_schedule/*.txt come from `rocprofv3 --kernel-trace` runs of ONE forward per configuration on that parent commit
(tools/tower_schedule_from_trace.py), never from the describe entry: a difference means the chooser picks another kernel than the
if-chain it replaced.  A trace knows streams, names, grids and workgroup sizes, not frames: the comparison is the per-stream order of
kernel names; the single-block kernels of bottleneck_wide.hip, which launch_bneck_wide picks by itself, are one name ("bneck_wide")."""
import ctypes
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tower_schedule", "*.txt")))
WIDE_BLOCK = {"bneck_halo_kernel", "bneck_halo64s_kernel", "bneck_halo128s_kernel", "bneck_half16_kernel", "bneck_wide_kernel"}
DTYPES = {"fp32": 0, "bf16": 1, "bf16x3": 2}

CHILD = r"""
import ctypes, sys
h = ctypes.CDLL(sys.argv[1])
h.ivosw_assess_describe.argtypes = [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(1 << 20)
rc = h.ivosw_assess_describe(*[int(v) for v in sys.argv[2:6]], buf, len(buf))
assert rc == 0, rc
sys.stdout.write(buf.value.decode())
"""


def read_golden(path):
    cfg, tune, rows = {}, {}, []
    for ln in open(path):
        if ln.startswith("# config:"):
            cfg = dict(kv.split("=") for kv in ln.split(":", 1)[1].split())
        elif ln.startswith("# tune:"):
            tune = dict(kv.split("=") for kv in ln.split(":", 1)[1].split())
        elif ln.strip() and not ln.startswith("#"):
            stream, name = ln.split()[:2]
            rows.append((int(stream), "bneck_wide" if name in WIDE_BLOCK else name))
    return cfg, tune, rows


def test_golden_schedules_cover_the_issue_configurations():
    assert len(FILES) >= 18, FILES


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_describe_matches_the_parent_trace(path):
    from ivos_w_amd import _lib as L
    if not L.available():
        import __graft_entry__ as g
        g.build()
    cfg, tune, want = read_golden(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("IVOSW_TUNE_")}
    env.update({"IVOSW_TUNE_" + k: v for k, v in tune.items()})
    r = subprocess.run([sys.executable, "-c", CHILD, L.LIB_PATH, str(DTYPES[cfg["precision"]]), cfg["B"], cfg["chunk"], cfg["tap_stage"]],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [(int(ln.split()[0]), ln.split()[1]) for ln in r.stdout.splitlines()]
    assert want and got == want, "\n".join(f"{i}: trace {w}  describe {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g)[:3000] + \
        f"\n(trace {len(want)} launches, describe {len(got)})"


def test_describe_argument_errors():
    from ivos_w_amd import _lib as L
    lib = L.lib()
    buf = ctypes.create_string_buffer(16)
    assert lib.ivosw_assess_describe(7, 8, 0, 0, buf, len(buf)) == -1
    assert lib.ivosw_assess_describe(L.BF16, 0, 0, 0, buf, len(buf)) == -1
    assert lib.ivosw_assess_describe(L.BF16, 16, 8, 4, buf, len(buf)) == -1 and b"taps" in lib.ivosw_last_error()
    assert lib.ivosw_assess_describe(L.BF16, 8, 0, 0, buf, len(buf)) != 0 and b"buffer" in lib.ivosw_last_error()      # too small: nothing written past cap
    assert L.assess_describe(L.BF16, 8)[0][1] == "stem_pool_kernel"


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 64])
def test_forward_enqueues_what_describe_lists(B):
    """bf16 at B = 8 (one stream) and B = 64 (two): the launches counted inside the profiler's spans of one forward pass are the lines
    the describe entry lists, so the description and the run cannot drift apart."""
    import numpy as np
    import torch
    from ivos_w_amd import _lib as L, synth
    from ivos_w_amd.models.assessment import AssessNet
    dev = torch.device("cuda:0")
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net.to(dev).eval()
    tf, tp = synth.assess_inputs(8, H=240, W=320, seed=5)
    ttf, ttp = torch.from_numpy(tf).to(dev).repeat(B // 8, 1, 1, 1), torch.from_numpy(tp).to(dev).repeat(B // 8, 1, 1)
    net(ttf, ttp)
    torch.cuda.synchronize()
    lib = L.lib()
    lines = L.assess_describe(L.BF16, B)
    assert {s for s, _, _, _ in lines} == ({0, 1} if lib.ivosw_assess_split(L.BF16, B, 0) else {0})
    tot, spans, cnt = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_int(0)
    L.check(lib.ivosw_profile_span_start())
    try:
        net(ttf, ttp)
    finally:
        L.check(lib.ivosw_profile_span_stop(ctypes.byref(tot), ctypes.byref(spans), ctypes.byref(cnt)))
    print(f"B {B}: {cnt.value} launches in {spans.value} spans, describe lists {len(lines)}")
    assert cnt.value == len(lines) and cnt.value > 0
