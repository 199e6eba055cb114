"""CPU: the host-only side of the boxed scribble robot (``ivosw_robot_skeleton_box``: any frame size, object 0) - the workspace
arithmetic, the argument checks that come before any device lookup, and the ``robot_background`` option."""
import ctypes

import numpy as np
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry

ERR_ARG = -1


def test_workspace_bytes_arithmetic():
    lib = L.lib()
    assert lib.ivosw_robot_box_workspace_bytes(480, 854, 3) == 0 and lib.ivosw_robot_skeleton_fits(480, 854) == 1
    for m in (1, 3, 65):
        assert lib.ivosw_robot_box_workspace_bytes(720, 1280, m) == m * 2 * 720 * 40 * 4
        assert lib.ivosw_robot_box_workspace_bytes(1080, 1920, m) == m * 2 * 1080 * 60 * 4
    assert lib.ivosw_robot_box_workspace_bytes(10224, 40, 1) == 0                       # the largest two-word-row size that fits
    assert lib.ivosw_robot_box_workspace_bytes(10225, 40, 2) == 2 * 2 * 10225 * 2 * 4
    assert lib.ivosw_robot_box_workspace_bytes(65535, 65535, 64) == 64 * 2 * 65535 * 2048 * 4       # beyond 2^31: the result is a long
    for H, W in ((0, 5), (5, 0), (-1, 5), (65536, 5), (5, 65536)):
        assert lib.ivosw_robot_box_workspace_bytes(H, W, 1) < 0
    assert lib.ivosw_robot_box_workspace_bytes(720, 1280, 0) < 0


def _call(**over):
    """ivosw_robot_skeleton_box on made-up HOST addresses (never a device pointer): every case below must be refused by the argument checks,
    which come before any pointer is used or looked up."""
    fake = lambda k: ctypes.c_void_p(0x1000 * (k + 1))
    units = np.ascontiguousarray(np.asarray(over.pop("rows", [(0, 1), (1, 2)]), np.int32))
    a = dict(gt=fake(0), pred=fake(1), n=2, H=720, W=1280, units=units.ctypes.data, m=len(units), cap=8, points=fake(2), counts=fake(3),
             iters=fake(4), skel=fake(5), ws=fake(6), ws_bytes=len(units) * 2 * 720 * 40 * 4)
    a.update(over)
    rc = L.lib().ivosw_robot_skeleton_box(a["gt"], a["pred"], a["n"], a["H"], a["W"], a["units"], a["m"], a["cap"], a["points"], a["counts"],
                                          a["iters"], a["skel"], a["ws"], a["ws_bytes"], None)
    return rc, L.lib().ivosw_last_error().decode()


def test_box_entry_refuses_at_the_argument_checks():
    need = 2 * 2 * 720 * 40 * 4
    cases = [(dict(gt=None), "null gt"), (dict(points=None), "null points"), (dict(counts=None), "null counts"), (dict(iters=None), "null iters"),
             (dict(units=None), "null units_host"), (dict(m=0), "m < 1"), (dict(m=-2), "m < 1"), (dict(cap=0), "cap < 1"), (dict(n=0), "n < 1"),
             (dict(H=0), "H outside [1, 65535]"), (dict(H=65536), "H outside"), (dict(W=0), "W outside [1, 65535]"), (dict(W=65536), "W outside"),
             (dict(rows=[(0, 1), (2, 1)]), "unit 1: frame 2 outside [0, 2)"), (dict(rows=[(-1, 1)]), "unit 0: frame -1 outside"),
             (dict(rows=[(0, 256)]), "unit 0: object 256 outside [0, 255]"), (dict(rows=[(0, 1), (1, -1)]), "unit 1: object -1 outside [0, 255]"),
             (dict(rows=[(0, 1), (1, 0)], pred=None), "unit 1: object 0"),
             (dict(ws=None), f"needs {need} bytes"), (dict(ws_bytes=need - 1), f"needs {need} bytes"), (dict(ws=None, ws_bytes=0), "H = 720, W = 1280")]
    for over, word in cases:
        rc, msg = _call(**over)
        assert rc == ERR_ARG and word in msg and msg.startswith("ivosw_robot_skeleton_box: "), (over, msg)
    rc, msg = _call(ws_bytes=need - 1)
    assert f"got {need - 1}" in msg and "230656" in msg and "163840" in msg, msg
    rc, msg = _call(rows=[(0, 0)], pred=None)
    assert "null pred" in msg, msg


def _cfg(**kw):
    return entry.parse_cli([f"{k}={v}" for k, v in kw.items()])


def test_robot_background_option_defaults_and_refusals():
    assert entry.DEFAULTS["robot_background"] is False
    assert entry.robot_background_option(_cfg()) is False and entry.robot_background_option({}) is False
    assert entry.robot_background_option(_cfg(scribbles="paths", robot="errors")) is False
    assert entry.robot_background_option(_cfg(scribbles="paths", robot="errors", robot_background="true")) is True
    assert entry.robot_background_option(_cfg(robot_background="false")) is False
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="robot_background must be true or false"):
            entry.robot_background_option(dict(robot="errors", scribbles="paths", robot_background=bad))
    for cfg in (dict(robot_background=True), dict(robot_background=True, robot="gt", scribbles="paths")):
        with pytest.raises(ValueError, match="needs robot=errors"):
            entry.robot_background_option(cfg)
    with pytest.raises(SystemExit, match="needs robot=errors"):
        _cfg(robot_background="true")
    with pytest.raises(SystemExit, match="needs robot=errors"):
        _cfg(robot_background="true", scribbles="paths")
    with pytest.raises(SystemExit, match="robot_background must be true or false"):
        _cfg(robot_background="maybe", scribbles="paths", robot="errors")


def test_session_keeps_the_flag_and_the_default_session_does_not_pass_it(monkeypatch):
    import torch
    from ivos_w_amd.utils import robot as R
    cfg = _cfg(seed=3)
    cfg.synth.n_sequences, cfg.synth.n_frames, cfg.synth.height, cfg.synth.width = 1, 4, 48, 64
    cfg.data.subset = "val"
    davis = entry.SyntheticDavis(cfg, torch.device("cpu"))
    seen = []
    monkeypatch.setattr(R, "interact", lambda *a, **k: seen.append(k) or [dict(path=[[0.5, 0.5]], object_id=1, start_time=0, end_time=0)])
    for flag, want in ((False, False), (True, True)):
        sess = entry.SyntheticSession(davis, "val", "J_AND_F", 2, "unused", seed=3, scribbles="paths", robot="errors", robot_background=flag)
        assert sess.next() and sess.robot_background is want
        sess.get_scribbles(only_last=True)
        assert ("background" in seen[-1]) is want and seen[-1].get("background", False) is want


def test_box_kernel_has_no_static_lds_and_no_scratch():
    """The plane-home rule counts two box planes and the 256 fixed bytes against the launch's dynamic LDS, so the code object must bring
    no LDS of its own; both plane homes are inlined into one kernel and must not spill (1024 threads: at most 128 registers)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    for path in (L.LIB_PATH, L.PROBE_LIB_PATH):
        rows = [r for n, r in kr.kernel_table(path).items() if "robot_skeleton_box_kernel" in n]
        assert len(rows) == 1 and rows[0]["lds"] == 0 and rows[0]["scratch"] == 0 and rows[0]["spill"] == 0 and rows[0]["vgpr"] <= 128, rows


def test_header_and_bindings_hold_the_new_symbols():
    from tests.test_cabi import declared_symbols
    assert {"ivosw_robot_skeleton_box", "ivosw_robot_box_workspace_bytes"} <= set(declared_symbols()) and \
        {"ivosw_robot_skeleton_box", "ivosw_robot_box_workspace_bytes"} <= set(L.SIGNATURES)
    assert "ivosw_robot_box_probe" in declared_symbols("ivosw_probe.h") and "ivosw_robot_box_probe" in L.PROBE_SIGNATURES
    assert declared_symbols() == sorted(L.SIGNATURES) and declared_symbols("ivosw_probe.h") == sorted(L.PROBE_SIGNATURES)
    assert not hasattr(ctypes.CDLL(L.LIB_PATH), "ivosw_robot_box_probe") and hasattr(ctypes.CDLL(L.PROBE_LIB_PATH), "ivosw_robot_box_probe")
    assert len(L.SIGNATURES["ivosw_robot_skeleton_box"][1]) == 15 and len(L.PROBE_SIGNATURES["ivosw_robot_box_probe"][1]) == 16
