"""CPU: the rules of the assessment-sample path as tests/qa_ref.py restates them - the threshold, the quantiser, the reference loop's
loss / diff - utils.misc.save_seg_preds with the quantiser patched to the restatement, and the save_probs / qa_report keys."""
import math
import os

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import entry, metrics
from ivos_w_amd.utils import misc, utils_agent
from tests import qa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_rule_for_all_bytes():
    """quality_assessment.py:190, 235: (np.array(png) / 255) > 0.8 - first true at 205, in float64 and, against the Python scalar, in float32."""
    q = np.arange(256)
    np.testing.assert_array_equal((q / 255) > 0.8, q >= 205)
    np.testing.assert_array_equal((q.astype(np.float32) / np.float32(255)) > 0.8, q >= 205)
    np.testing.assert_array_equal((torch.arange(256, dtype=torch.float32) / 255 > 0.8).numpy(), q >= 205)
    np.testing.assert_array_equal((torch.arange(256, dtype=torch.float64) / 255 > 0.8).numpy(), q >= 205)
    assert metrics.QA_THRESHOLD == R.THR == 205


def _byte_by_hand(v):
    """One value through the rule with Python scalars: the float32 product exactly as a double, round() (half to even), the clamp."""
    t = float(np.float32(v) * np.float32(255.0)) if not np.isinf(v) else float(v) * 1.0
    if math.isnan(t):
        return 0
    if math.isinf(t):
        return 255 if t > 0 else 0
    return min(max(round(t), 0), 255)


def test_quantiser_restatement_on_the_deciding_grid():
    g = R.value_grid()
    assert g.dtype == np.float32 and g.size > 4 * 256
    with np.errstate(over="ignore"):
        want = np.asarray([_byte_by_hand(v) for v in g], dtype=np.uint8)
    got = R.quantize(g)
    np.testing.assert_array_equal(got, want)
    with np.errstate(invalid="ignore", over="ignore"):
        np.testing.assert_array_equal(got, np.clip(np.nan_to_num(np.rint(g * np.float32(255)), nan=0.0, posinf=255, neginf=0), 0, 255).astype(np.uint8))
    assert set(got.tolist()) == set(range(256))                          # every byte is reached
    # ties go to the even byte: the grid holds products that are exactly k + 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (g * np.float32(255)).astype(np.float64)
        ties = np.isfinite(prod) & (prod - np.floor(prod) == 0.5) & (prod > 0) & (prod < 255)
    assert ties.sum() >= 8 and (got[ties] % 2 == 0).all()
    special = dict(zip(["-0.0", "neg", "one", "above", "inf", "-inf", "nan"],
                       R.quantize(np.asarray([-0.0, -0.3, 1.0, 1.002, np.inf, -np.inf, np.nan], np.float32)).tolist()))
    assert special == {"-0.0": 0, "neg": 0, "one": 255, "above": 255, "inf": 255, "-inf": 0, "nan": 0}
    np.testing.assert_array_equal(R.quantize(np.arange(256, dtype=np.float32) / np.float32(255)), np.arange(256))      # bytes / 255 come back


def test_quantize_probs_layout_and_channel_zero():
    a = R.fill((3, 4, 5, 7))
    a[:, 0] = np.nan
    q = R.quantize_probs(a, 3)
    assert q.shape == (3, 3, 5, 7) and q.dtype == np.uint8
    for o in range(3):
        for f in range(3):
            np.testing.assert_array_equal(q[o, f], R.quantize(a[f, o + 1]))
    np.testing.assert_array_equal(R.quantize_probs(a, 2), q[:2])


@pytest.mark.parametrize("units, p_valid", [(1, 1.0), (7, 1.0), (7, 0.5), (7, 0.0), (300, 0.8)])
def test_report_rule_is_the_reference_loop(units, p_valid):
    rng = np.random.default_rng(units * 10 + int(p_valid * 4))
    scores = rng.random(units).astype(np.float32)
    target = rng.random(units)                                            # float64, as sequence_metric returns it
    target[rng.random(units) < 0.2] = 1.0
    valid = (rng.random(units) < p_valid).astype(np.uint8)
    got, want = R.report(scores, target, valid), R.reference_loop(scores, target, valid)
    assert got[2] == want[2] == int(valid.sum())
    assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and np.float32(got[1]).tobytes() == np.float32(want[1]).tobytes()
    if units == 300:                                                      # the order matters: the fp32 sum of the same terms sorted differs
        e = (scores - target.astype(np.float32))[valid > 0]
        assert np.float32(np.sort(e * e).sum() / np.float32(len(e))).tobytes() != got[0].tobytes() or \
            np.float32((e * e).astype(np.float64).sum() / len(e)).tobytes() != got[0].tobytes()
    if p_valid == 0.0:
        assert got == (0, 0, 0)


def test_unit_targets_order_and_expressions():
    """counts are frame-major [N, O, 6]; the targets come out object-major, by metrics.py's host expressions."""
    counts = np.zeros((2, 3, 6), np.int64)
    counts[0, 0] = [3, 4, 5, 6, 2, 3]
    counts[1, 0] = [0, 0, 0, 0, 0, 0]          # empty union: J = 1, F = 1, not valid
    counts[0, 1] = [0, 9, 0, 4, 0, 0]          # no pred boundary
    counts[1, 1] = [1, 9, 4, 0, 0, 0]          # no gt boundary
    counts[0, 2] = [2, 7, 3, 3, 0, 0]          # precision + recall == 0
    counts[1, 2] = [7, 7, 5, 5, 5, 5]
    for metric in ("J", "F", "J_AND_F"):
        t, v = R.unit_targets(counts, metric)
        assert t.shape == (6,) and v.tolist() == [1, 0, 1, 1, 1, 1]
        j, f = metrics._jaccard_from(counts), metrics._f_from(counts)
        full = {"J": j, "F": f, "J_AND_F": .5 * j + .5 * f}[metric]
        assert [t[o * 2 + n] for o in range(3) for n in range(2)] == [full[n, o] for o in range(3) for n in range(2)]
    t, _ = R.unit_targets(counts, "J")
    assert t.tolist() == [0.75, 1.0, 0.0, 1 / 9, 2 / 7, 1.0]


# ------------------------------------------------------------------------------------------------ save_seg_preds
def _read_gray(path):
    if path.endswith(".png"):
        from PIL import Image
        im = Image.open(path)
        assert im.mode == "L"
        return np.asarray(im)
    raw = open(path, "rb").read()
    head, dims, top, body = raw.split(b"\n", 3)
    assert head == b"P5" and top == b"255"
    w, h = (int(v) for v in dims.split())
    return np.frombuffer(body, np.uint8).reshape(h, w)


@pytest.fixture
def host_quantiser(monkeypatch):
    calls = []

    def fake(all_P, n_objects):
        calls.append(int(n_objects))
        p = all_P.all_P if hasattr(all_P, "all_P") else all_P
        return torch.from_numpy(R.quantize_probs(p, n_objects))
    monkeypatch.setattr(metrics, "quantize_probs", fake)
    return calls


def test_save_seg_preds_paths_names_and_bytes(tmp_path, host_quantiser):
    a = R.fill((3, 3, 5, 7), np.random.default_rng(1))
    a[:, 0] = np.nan                                                      # channel 0 is neither read nor written
    meta = dict(sequence="bear", n_interaction=2, scribble_iter=1)
    paths = misc.save_seg_preds(torch.from_numpy(a), meta, str(tmp_path))
    assert host_quantiser == [2]                                          # one quantise call for the whole all_P
    base = os.path.join(str(tmp_path), "interaction-2", "scribble-1", "bear", "probs")
    ext = os.path.splitext(paths[0])[1]
    assert ext in (".png", ".pgm")
    assert paths == [os.path.join(base, str(o), f"{i:05d}{ext}") for o in (1, 2) for i in range(3)]
    assert sorted(os.listdir(base)) == ["1", "2"]                         # no directory for channel 0
    assert sorted(os.listdir(os.path.join(base, "1"))) == [f"0000{i}{ext}" for i in range(3)]
    q = R.quantize_probs(a, 2)
    for k, p in enumerate(paths):
        np.testing.assert_array_equal(_read_gray(p), q[k // 3, k % 3], err_msg=p)
    # the already quantised tensor goes straight to the files
    again = misc.save_seg_preds(torch.from_numpy(q), dict(meta, n_interaction=3), str(tmp_path))
    assert host_quantiser == [2] and len(again) == 6
    np.testing.assert_array_equal(_read_gray(again[-1]), q[1, 2])
    with pytest.raises(ValueError, match="uint8"):
        misc.save_seg_preds(torch.zeros(3, 5, 7, dtype=torch.uint8), meta, str(tmp_path))


def test_save_seg_preds_pgm_fallback(tmp_path, host_quantiser, monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("PIL is hidden for this test")
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    a = R.fill((2, 2, 4, 6))
    paths = misc.save_seg_preds(torch.from_numpy(a), dict(sequence="s", n_interaction=1, scribble_iter=1), str(tmp_path))
    monkeypatch.setattr(builtins, "__import__", real_import)
    assert [os.path.basename(p) for p in paths] == ["00000.pgm", "00001.pgm"]
    raw = open(paths[1], "rb").read()
    assert raw.startswith(b"P5\n6 4\n255\n") and len(raw) == len(b"P5\n6 4\n255\n") + 24
    np.testing.assert_array_equal(_read_gray(paths[1]), R.quantize(a[1, 1]))


# ------------------------------------------------------------------------------------------------ keys
def test_keys_default_off_and_parse():
    assert entry.DEFAULTS["save_probs"] is False and entry.DEFAULTS["qa_report"] is False
    assert entry.qa_option({}) == (False, False)
    cfg = entry.parse_cli([])
    assert (cfg.save_probs, cfg.qa_report) == (False, False) == entry.qa_option(cfg)
    cfg = entry.parse_cli(["with", "setting=wild", "method=ours", "qa_report=true", "save_probs=true"])
    assert entry.qa_option(cfg) == (True, True)
    assert entry.qa_option(entry.parse_cli(["with", "setting=wild", "method=worst", "qa_report=true"])) == (False, True)
    assert entry.qa_option(entry.parse_cli(["with", "setting=oracle", "save_probs=true"])) == (True, False)
    assert entry.qa_option(entry.parse_cli(["with", "masks=labels", "qa_report=true"])) == (False, True)       # scores the one-hot planes


def test_keys_refusals():
    for bad in (["setting=oracle"], ["method=random"], ["method=linspace"], ["setting=oracle", "method=worst"]):
        with pytest.raises(SystemExit, match="qa_report=true needs AssessNet's scores"):
            entry.parse_cli(["with", "qa_report=true"] + bad)
    with pytest.raises(SystemExit, match="save_probs=true is refused under masks=labels"):
        entry.parse_cli(["with", "save_probs=true", "masks=labels"])
    for key in ("save_probs", "qa_report"):
        for bad in ("1", "yes", "none", "2.5"):
            with pytest.raises(SystemExit, match=f"{key} must be true or false"):
                entry.parse_cli(["with", f"{key}={bad}"])
    cfg = entry.parse_cli(["with", "synthetic=1"])                        # run_eval refuses before any work
    cfg.qa_report, cfg.setting = True, "oracle"
    with pytest.raises(ValueError, match="qa_report"):
        entry.run_eval(cfg)
    cfg = entry.parse_cli(["with", "synthetic=1"])
    cfg.save_probs, cfg.masks = True, "labels"
    with pytest.raises(ValueError, match="save_probs"):
        entry.run_eval(cfg)


class _Loop:
    """run_eval's loop on the CPU: its collaborators that need the GPU are stubbed (the synthetic data and the store live on the host, the
    segmentation, the metric and the recommender are stand-ins), every call is logged, and the loop itself is the real one."""

    def __init__(self, monkeypatch, tmp_path):
        from ivos_w_amd.utils import utils_manet
        self.log, self.tmp = [], tmp_path
        cpu = torch.device("cpu")
        real_davis, real_store = entry.SyntheticDavis, utils_manet.ProbStore
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(entry, "SyntheticDavis", lambda cfg, device: real_davis(cfg, cpu))
        monkeypatch.setattr(utils_manet, "ProbStore", lambda n, c, h, w, device: real_store(n, c, h, w, cpu))

        class Agent:
            def set_eval(self):
                pass
        monkeypatch.setattr(entry, "build_hot_path", lambda cfg, device, need: (Agent(), object() if need else None))

        def segment(vos, davis, seq, n_objects, annotated, store):
            self.log.append(("segment", seq, tuple(annotated)))
            gt = davis.load_annotations(seq)
            store.labels_u8.copy_(gt)
            for c in range(n_objects + 1):
                store.buf[c] = torch.where(gt == c, 0.9, 0.1 / n_objects)
            return store.labels_u8, store.all_P
        monkeypatch.setattr(entry, "_segment", segment)

        def sequence_metric(metric, gt, pred, n_objects, **kw):
            self.log.append(("metric", metric, int(n_objects)))
            return np.linspace(0.5, 0.9, int(gt.shape[0]))
        monkeypatch.setattr(misc, "sequence_metric", sequence_metric)

        def recommend(cfg, assess_net, agent, device, requests):
            self.log.append(("recommend", len(requests), requests[0]["n_frame"]))
            if utils_agent.score_tap is not None:                        # what the assessment pass would leave for the report
                utils_agent.score_tap.append(torch.zeros(requests[0]["n_objects"], requests[0]["n_frame"]))
            return [np.asarray([len(self.log) % requests[0]["n_frame"]])]
        monkeypatch.setattr(utils_agent, "recommend_candidates", recommend)

    def run(self, name, extra=(), drop=False):
        cfg = entry.parse_cli(["with", "synthetic=1", "setting=wild", "method=ours", "synth.n_sequences=2", "synth.n_frames=4", "synth.height=12",
                               "synth.width=20", "eval_max_nb_interactions=2", f"report_save_dir={self.tmp}/{name}",
                               f"agent.save_result_dir={self.tmp}/{name}_probs"] + list(extra))
        if drop:
            del cfg["save_probs"], cfg["qa_report"]
        del self.log[:]
        out = entry.run_eval(cfg, "MANet")
        return out, list(self.log), open(os.path.join(out["report_dir"], "summary.json"), "rb").read()


def test_without_the_keys_the_loop_is_untouched(monkeypatch, tmp_path, capsys, host_quantiser):
    """Both keys absent or false: no QaSession is made, the score tap stays None, and the loop's calls, stdout and summary.json are those
    of a run with the keys on minus what the keys add."""
    loop = _Loop(monkeypatch, tmp_path)
    real_session = entry.QaSession
    monkeypatch.setattr(entry, "QaSession", lambda *a, **k: pytest.fail("QaSession was made without a key"))
    assert utils_agent.score_tap is None
    _, calls_absent, sum_absent = loop.run("absent", drop=True)
    text_absent = capsys.readouterr().out
    _, calls_off, sum_off = loop.run("off", ["save_probs=false", "qa_report=false"])
    text_off = capsys.readouterr().out
    assert utils_agent.score_tap is None and host_quantiser == []
    assert calls_absent == calls_off and len([c for c in calls_off if c[0] == "segment"]) == 4
    assert sum_absent == sum_off and "qa" not in sum_off.decode()
    strip = lambda t, k: t.replace(f"{tmp_path}/{k}", "DIR")
    import re
    times = lambda t: re.sub(r"(rec_time:|recommend_frame avg )\s*[0-9.]+", r"\1T", t)
    assert times(strip(text_absent, "absent")) == times(strip(text_off, "off")) and "qa_" not in text_off and "save_probs" not in text_off
    assert not os.path.exists(f"{tmp_path}/off_probs")
    # the keys on: the same calls in the same order, one report per interaction, the files of every interaction
    seen = []

    class Spy(real_session):
        def after(self, sequence, visit, n_interaction, gt_masks, labels, all_P, n_objects, device):
            seen.append((sequence, visit, n_interaction, n_objects))
            assert len(utils_agent.score_tap) == 1                         # this interaction's scores, nothing older
            return super().after(sequence, visit, n_interaction, gt_masks, labels, all_P, n_objects, device)
    monkeypatch.setattr(entry, "QaSession", Spy)
    monkeypatch.setattr(utils_agent, "assess_report", lambda videos, scores, metric: (np.asarray([[0.25, 0.5, 3]], np.float32), None))
    out, calls_on, sum_on = loop.run("on", ["save_probs=true", "qa_report=true"])
    text_on = capsys.readouterr().out
    assert calls_on == calls_off and utils_agent.score_tap is None
    assert [s[2] for s in seen] == [1, 2, 1, 2] and len(host_quantiser) == 4
    import json
    on = json.loads(sum_on)
    assert on["qa"] == {"loss": 0.25, "diff": 0.5, "valid": 12, "units": sum(4 * s[3] for s in seen)}
    assert {k: v for k, v in on.items() if k != "qa"} == json.loads(sum_off)
    lines_on = [ln for ln in text_on.splitlines() if ln.startswith("avg_")]
    assert len(lines_on) == 4 and all("corr: " in ln and " qa_loss: 0.2500 qa_diff: 0.5000 valid: 3/" in ln for ln in lines_on)
    assert [times(re.sub(r"qa_loss.*valid: \d+/\d+ ", "", ln)) for ln in lines_on] == \
        [times(ln) for ln in text_off.splitlines() if ln.startswith("avg_")]
    files = [os.path.join(d, f) for d, _, fs in os.walk(f"{tmp_path}/on_probs") for f in fs]
    assert len(files) == on["qa"]["units"]


def test_the_score_tap_is_released_when_the_loop_raises(monkeypatch, tmp_path, host_quantiser):
    loop = _Loop(monkeypatch, tmp_path)
    monkeypatch.setattr(utils_agent, "assess_report", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError, match="boom"):
        loop.run("raises", ["qa_report=true"])
    assert utils_agent.score_tap is None

    class Fake:
        def detach(self):
            pytest.fail("a score tensor was copied although nobody asked")
    utils_agent._tap(Fake())


def test_generate_data_fixes_its_keys_and_says_so(monkeypatch, capsys):
    got = {}
    monkeypatch.setattr(entry, "run_eval", lambda cfg, backbone: got.update(cfg=cfg, backbone=backbone) or {"ok": 1})
    assert entry.main_generate(["with", "setting=wild", "method=worst", "agent.save_result_dir=somewhere"]) == {"ok": 1}
    cfg = got["cfg"]
    assert (cfg.save_probs, cfg.synthetic, cfg.agent.save_result_dir, got["backbone"]) == (True, 1, "somewhere", "MANet")
    text = capsys.readouterr().out
    assert "generate_data: the synthetic back end" in text and "save_probs=true -> somewhere" in text
    for bad in ("save_probs=false", "synthetic=0", "synthetic=-1"):
        with pytest.raises(SystemExit, match="save_probs=true synthetic=1 are fixed"):
            entry.main_generate(["with", bad])
    with pytest.raises(SystemExit, match="masks=labels"):
        entry.main_generate(["with", "masks=labels"])
    src = open(os.path.join(ROOT, "generate_data.py")).read()
    assert "entry.main_generate()" in src


def test_the_keys_are_refused_for_training():
    for key in ("save_probs", "qa_report"):
        with pytest.raises(SystemExit, match="belong to the eval scripts"):
            entry.parse_cli(["with", "setting=wild", "method=ours", f"{key}=true"], phase="train")
    assert entry.qa_option(entry.parse_cli([], phase="train")) == (False, False)


def test_header_bindings_and_documents_agree():
    header = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for name in ("ivosw_qa_quantize", "ivosw_qa_counts_ws_bytes", "ivosw_qa_counts_videos", "ivosw_qa_targets"):
        assert name in L.SIGNATURES and name + "(" in header
    for cite in ("utils/misc.py:165-181", "quality_assessment.py:178-196, 235-263", "restated, not recorded", "IVOSW_QA_SCALAR"):
        assert cite in header, cite
    from ivos_w_amd import build
    assert "qa.hip" in build.SOURCES
    import ctypes
    assert ctypes.sizeof(L.QaVideo) == 72 and L.QaVideo.thr.offset == 68 and L.QaVideo.bound_pix.offset == 64
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ivosw_qa_quantize" in text and "qa_report" in text, doc
    assert os.path.exists(os.path.join(ROOT, "generate_data.py"))


def test_wrappers_refuse_before_touching_the_gpu(monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the library was reached"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.quantize_probs(torch.zeros(2, 3, 4, 4), 2)
    with pytest.raises(ValueError, match="metric must be"):
        metrics.qa_targets([(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 1, 2, 2), np.uint8), 1)], "IoU")
    with pytest.raises(ValueError, match="at least one video"):
        metrics.qa_counts([])
    with pytest.raises(ValueError, match="thr must be a byte"):
        metrics.qa_counts([(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 1, 2, 2), np.uint8), 1)], thr=256)
