"""The ``robot_paths`` option (host | device): its refusals, the untouched default, the host-only side of ``ivosw_robot_paths`` (the cap
arithmetic, the argument checks that come before any device lookup, the kernel's resources) and - on the GPU - a short synthetic
``run_eval`` whose device run gives the summary and the masks of the host run."""
import ctypes
import json
import os

import numpy as np
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry

ERR_ARG = -1


def _cfg(**kw):
    return entry.parse_cli([f"{k}={v}" for k, v in kw.items()])


def test_robot_paths_option_defaults_and_refusals():
    assert entry.DEFAULTS["robot_paths"] == "host"
    assert entry.robot_paths_option({}) == "host" and entry.robot_paths_option(_cfg()) == "host"
    assert entry.robot_paths_option(_cfg(scribbles="paths", robot="errors", robot_paths="device")) == "device"
    assert entry.robot_paths_option(_cfg(scribbles="paths", robot="errors", robot_paths="host")) == "host"
    for bad in ("gpu", 1, None, True, "Device"):
        with pytest.raises(ValueError, match="robot_paths must be 'host' or 'device'"):
            entry.robot_paths_option(dict(robot="errors", scribbles="paths", robot_paths=bad))
    for cfg in (dict(robot_paths="device"), dict(robot_paths="device", robot="gt", scribbles="paths")):
        with pytest.raises(ValueError, match="needs robot=errors"):
            entry.robot_paths_option(cfg)
    with pytest.raises(SystemExit, match="robot_paths must be 'host' or 'device'"):
        _cfg(robot_paths="gpu", scribbles="paths", robot="errors")
    with pytest.raises(SystemExit, match="needs robot=errors"):
        _cfg(robot_paths="device", scribbles="paths")
    with pytest.raises(ValueError, match="robot_paths must be"):       # run_eval refuses before anything runs (no device is asked for)
        cfg = _cfg(scribbles="paths", robot="errors")
        cfg.robot_paths = "gpu"
        entry.run_eval(cfg)


def test_the_default_session_does_not_know_the_option(monkeypatch):
    """robot_paths=host: the session calls ``interact`` exactly as it did (no new keyword) and keeps no device paths."""
    import torch
    from ivos_w_amd.utils import robot as R
    cfg = _cfg(seed=3)
    cfg.synth.n_sequences, cfg.synth.n_frames, cfg.synth.height, cfg.synth.width = 1, 4, 48, 64
    cfg.data.subset = "val"
    davis = entry.SyntheticDavis(cfg, torch.device("cpu"))
    seen = []
    monkeypatch.setattr(R, "interact", lambda *a, **k: seen.append(k) or [dict(path=[[0.5, 0.5]], object_id=1, start_time=0, end_time=0)])
    monkeypatch.setattr(R, "interact_device", lambda *a, **k: pytest.fail("the host session reached interact_device"))
    for kw in (dict(), dict(robot_paths="host")):
        sess = entry.SyntheticSession(davis, "val", "J_AND_F", 2, "unused", seed=3, scribbles="paths", robot="errors", **kw)
        assert sess.next() and sess.robot_paths == "host"
        sess.get_scribbles(only_last=True)
        assert sorted(seen[-1]) == ["min_nb_nodes", "nb_points"] and sess.device_paths is None and sess.drew == "errors"


def _call(**over):
    """ivosw_robot_paths on made-up HOST addresses (never a device pointer): every case must be refused by the argument checks, which come
    before any pointer is used or looked up."""
    fake = lambda k: ctypes.c_void_p(0x1000 * (k + 1))
    a = dict(points=fake(0), counts=fake(1), m=2, cap=64, H=480, W=854, min_nb_nodes=4, max_paths=2, nb_points=8, slot=8, nodes=fake(2),
             lens=fake(3), status=fake(4))
    a.update(over)
    rc = L.lib().ivosw_robot_paths(a["points"], a["counts"], a["m"], a["cap"], a["H"], a["W"], a["min_nb_nodes"], a["max_paths"], a["nb_points"],
                                   a["slot"], a["nodes"], a["lens"], a["status"], None)
    return rc, L.lib().ivosw_last_error().decode()


def test_entry_refuses_at_the_argument_checks_and_the_cap_arithmetic():
    cmax = L.lib().ivosw_robot_paths_max_cap()
    assert cmax >= 4096 and 36 * cmax + 256 <= 160 * 1024 < 36 * (cmax + 1) + 256
    cases = [(dict(points=None), "null points"), (dict(counts=None), "null counts"), (dict(nodes=None), "null nodes"),
             (dict(lens=None), "null lens"), (dict(status=None), "null status"), (dict(m=0), "m < 1"), (dict(m=-1), "m < 1"),
             (dict(cap=0), "cap 0 outside"), (dict(cap=cmax + 1), f"cap {cmax + 1} outside [1, {cmax}]"), (dict(H=0), "H outside [1, 65535]"),
             (dict(H=65536), "H outside"), (dict(W=0), "W outside [1, 65535]"), (dict(W=65536), "W outside"),
             (dict(min_nb_nodes=0), "min_nb_nodes < 1"), (dict(max_paths=0), "max_paths outside [1, 8]"), (dict(max_paths=9), "max_paths outside"),
             (dict(slot=0), "slot outside [1, cap]"), (dict(slot=65), "slot outside [1, cap]"), (dict(nb_points=9), "nb_points > slot"),
             (dict(nodes=ctypes.c_void_p(0x3004)), "nodes off the 8-byte grid")]
    for over, word in cases:
        rc, msg = _call(**over)
        assert rc == ERR_ARG and word in msg and msg.startswith("ivosw_robot_paths: "), (over, msg)


def test_paths_kernels_have_no_static_lds_and_no_scratch():
    """The cap limit counts 36 bytes per node and 256 fixed bytes against the 160 KB of one workgroup, so the code objects must bring no LDS
    of their own; nothing may spill (the 1024-thread form has at most 128 registers)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    rows = [r for n, r in kr.kernel_table(L.LIB_PATH).items() if "robot_paths_kernel" in n]
    assert len(rows) == 3 and all(r["lds"] == 0 and r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 128 for r in rows), rows


def test_header_and_bindings_hold_the_new_symbols():
    from tests.test_cabi import declared_symbols
    new = {"ivosw_robot_paths", "ivosw_robot_paths_max_cap"}
    assert new <= set(declared_symbols()) and new <= set(L.SIGNATURES) and len(L.SIGNATURES["ivosw_robot_paths"][1]) == 14
    assert declared_symbols() == sorted(L.SIGNATURES)


COMMON = ["with", "synthetic=1", "setting=oracle", "method=worst", "seed=0", "synth.n_sequences=1", "synth.n_frames=16", "synth.height=48",
          "synth.width=64", "eval_max_nb_interactions=4", "scribbles=paths", "robot=errors"]


def _run(tmp_path, name, capsys, monkeypatch, *extra):
    """One short synthetic run: (summary.json, the submitted masks, the log's avg_ lines without their wall-clock figure)."""
    masks = []
    submit = entry.SyntheticSession.submit_masks

    def spy(self, m, next_scribble_frame_candidates=None):
        masks.append(np.asarray(m.cpu()).copy())
        return submit(self, m, next_scribble_frame_candidates)
    with monkeypatch.context() as mp:
        mp.setattr(entry.SyntheticSession, "submit_masks", spy)
        out = entry.run_eval(entry.parse_cli(COMMON + [f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/{name}"] + list(extra)), "MANet")
    with open(os.path.join(out["report_dir"], "summary.json")) as fp:
        on_disk = json.load(fp)
    lines = [ln.split("rec_time")[0] + ln.split("ms", 1)[-1] for ln in capsys.readouterr().out.splitlines() if ln.startswith("avg_")]
    return on_disk, masks, lines


@pytest.mark.gpu
def test_device_run_gives_the_summary_and_masks_of_the_host_run(tmp_path, capsys, monkeypatch):
    plain = _run(tmp_path, "plain", capsys, monkeypatch)
    host = _run(tmp_path, "host", capsys, monkeypatch, "robot_paths=host")
    device = _run(tmp_path, "device", capsys, monkeypatch, "robot_paths=device")
    assert plain[0] == host[0] and plain[2] == host[2] and len(plain[2]) == 4          # the default run is the run without the key
    assert all("robot: " in ln and "device paths" not in ln for ln in host[2])
    assert device[0] == host[0] and len(device[1]) == len(host[1]) == 4
    for a, b in zip(device[1], host[1]):
        np.testing.assert_array_equal(a, b)
    assert sum("robot: errors (device paths)" in ln for ln in device[2]) >= 2
    assert [ln.replace("(device paths) ", "") for ln in device[2]] == host[2]
