"""Augmented assessment samples, the host side (no GPU): the numpy restatement of the sampling rule against hand-checked cases, the byte
conversion for all 256 bytes, the draws of datasets/transforms_assess.py against the reference's formulas written out here, the
composed maps against a step-by-step float64 composition, and the qa_augment key."""
import ctypes
import json
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.datasets import transforms_assess as T
from ivos_w_amd.utils import utils_agent
from tests import augment_ref as R
from tests.test_qa_option import _Loop, host_quantiser  # noqa: F401  (run_eval's loop on the CPU, and the fixture it needs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _video(H, W, n=2, O=2, seed=0, u8=False):
    g = np.random.RandomState(seed)
    frames = g.randint(0, 256, (n, H, W, 4)).astype(np.uint8) if u8 else g.rand(n, 3, H, W).astype(F32)
    return dict(frames=frames, gt=g.randint(0, O + 1, (n, H, W)).astype(np.uint8), planes=g.randint(0, 256, (O, n, H, W)).astype(np.uint8),
                obj_ids=list(range(1, O + 1)))


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_identity_returns_the_source_bits():
    for u8 in (False, True):
        v = _video(5, 7, u8=u8)
        out = R.augment([v], [dict(v=0, f=1, o=1, post=R.IDENTITY)], 5, 7)
        want = R.frame_planes(v["frames"], 1)
        assert out["img"][0].tobytes() == want.tobytes()
        assert out["prob"][0].tobytes() == (v["planes"][1, 1].astype(F32) / F32(255)).tobytes()
        np.testing.assert_array_equal(out["mask"][0], np.where(v["planes"][1, 1] >= 205, 255, 0))
        np.testing.assert_array_equal(out["label"][0], v["gt"][1] == 2)
        assert out["chosen"][0] == 0


def test_flip_and_integer_crop_copy_exactly():
    v = _video(6, 9)
    flip = R.augment([v], [dict(v=0, f=0, o=0, post=(-1., 0., 8., 0., 1., 0.))], 6, 9)
    assert flip["img"][0].tobytes() == np.ascontiguousarray(v["frames"][0][..., ::-1]).tobytes()
    np.testing.assert_array_equal(flip["label"][0], (v["gt"][0] == 1)[:, ::-1])
    np.testing.assert_array_equal(flip["prob"][0], (v["planes"][0, 0].astype(F32) / F32(255))[:, ::-1])
    crop = R.augment([v], [dict(v=0, f=0, o=0, post=(1., 0., 2., 0., 1., 1.))], 4, 5)
    assert crop["img"][0].tobytes() == np.ascontiguousarray(v["frames"][0][:, 1:5, 2:7]).tobytes()
    np.testing.assert_array_equal(crop["label"][0], (v["gt"][0] == 1)[1:5, 2:7])


def test_half_pixel_shift_by_hand_and_the_zero_border():
    src = np.array([[0.25, 0.75], [0.5, 1.0]], dtype=F32)
    got = R.bilinear(src, (1., 0., 0.5, 0., 1., 0.), 2, 2)                 # sx = x + .5: columns (0 + 1) / 2 and (1 + outside) / 2
    np.testing.assert_array_equal(got, np.array([[0.5, 0.375], [0.75, 0.5]], dtype=F32))
    got = R.bilinear(src, (1., 0., 0.5, 0., 1., 0.5), 2, 2)
    np.testing.assert_array_equal(got, np.array([[0.625, 0.4375], [0.375, 0.25]], dtype=F32))
    # taps at -1 and W read as 0: sx = x - 1 puts source column -1 under x = 0; sx = x + 1 puts column W under x = W - 1
    np.testing.assert_array_equal(R.bilinear(src, (1., 0., -1., 0., 1., 0.), 2, 2), np.array([[0., 0.25], [0., 0.5]], dtype=F32))
    np.testing.assert_array_equal(R.bilinear(src, (1., 0., 1., 0., 1., 0.), 2, 2), np.array([[0.75, 0.], [1.0, 0.]], dtype=F32))
    np.testing.assert_array_equal(R.bilinear(src, (1., 0., -0.5, 0., 1., 0.), 2, 2), np.array([[0.125, 0.5], [0.25, 0.75]], dtype=F32))
    gt = np.array([[1, 1], [1, 1]], dtype=np.uint8)
    np.testing.assert_array_equal(R.warp_label(gt, 1, (1., 0., -0.5, 0., 1., 0.), 2, 2), [[1, 1], [1, 1]])    # floor(-.5 + .5) = 0: inside
    np.testing.assert_array_equal(R.warp_label(gt, 1, (1., 0., -0.75, 0., 1., 0.), 2, 2), [[0, 1], [0, 1]])
    np.testing.assert_array_equal(R.warp_label(gt, 1, (1., 0., 0.5, 0., 1., 0.), 2, 2), [[1, 0], [1, 0]])     # floor(1.5 + .5) = 2 = W: outside


def test_photometric_order_and_clips():
    v = np.array([0.0, 0.5, 0.99, 1.0], dtype=F32)
    np.testing.assert_array_equal(R.photometric(v, 0.02, 1.5), np.clip(np.clip(v + F32(0.02), 0, 1) * F32(1.5), 0, 1).astype(F32))
    np.testing.assert_array_equal(R.photometric(v, -0.6, 1.0), np.array([0., 0., F32(0.99) + F32(-0.6), F32(1.0) + F32(-0.6)], dtype=F32))
    assert R.photometric(v, 0.5, 1.0)[2] == 1.0 and R.photometric(v, 0.0, 3.0)[1] == 1.0


def test_byte_conversion_for_all_bytes():
    b = np.arange(256)
    f = b.astype(F32) / F32(255.0)
    assert f.dtype == F32
    np.testing.assert_array_equal(f, (b.astype(np.float64) / 255).astype(F32))
    assert int(np.argmax(f > F32(0.8))) == 205 and not (f[:205] > F32(0.8)).any()
    from ivos_w_amd import metrics
    assert metrics.QA_THRESHOLD == 205


def test_selection_rule_of_the_restatement():
    gt = np.zeros((1, 6, 6), np.uint8)
    gt[0, 2:4, 2:4] = 1
    v = dict(frames=np.zeros((1, 3, 6, 6), F32), gt=gt, planes=np.zeros((1, 1, 6, 6), np.uint8), obj_ids=[1])
    away, stay = (1., 0., 100., 0., 1., 0.), (1., 0., 1., 0., 1., 0.)
    assert R.augment([v], [dict(v=0, f=0, o=0, cands=[away, away, stay], post=R.IDENTITY)], 6, 6)["chosen"][0] == 2
    out = R.augment([v], [dict(v=0, f=0, o=0, cands=[away] * 12, post=R.IDENTITY)], 6, 6)
    assert out["chosen"][0] == 12
    np.testing.assert_array_equal(out["label"][0], gt[0])


# ------------------------------------------------------------------------------------------------ the draws
def test_draws_equal_the_reference_formulas():
    sizes = [(20, 12)] * 5
    random.seed(7)
    np.random.seed(7)
    flips, _ = T.RandomHorizontalFlip().draw(sizes)
    noise = T.AdditiveNoise(delta=5.0).draw(5)
    contrast = T.RandomContrast(0.97, 1.03).draw(5)
    crops, out_sizes = T.RandomCrop(patch_size=8).draw(sizes)
    random.seed(7)
    np.random.seed(7)
    want_flip = [random.random() < 0.5 for _ in range(5)]
    want_noise = [np.random.uniform(-5.0 / 255., 5.0 / 255.) for _ in range(5)]
    want_contrast = [np.random.uniform(0.97, 1.03) for _ in range(5)]
    want_crop = []
    for _ in range(5):
        h_start = random.randint(0, 12 - 8)
        want_crop.append((random.randint(0, 20 - 8), h_start))
    for m, fl in zip(flips, want_flip):
        np.testing.assert_array_equal(m, T.flip_map(20) if fl else np.eye(3))
    np.testing.assert_array_equal(T.flip_map(20)[0], [-1., 0., 19.])
    assert noise == want_noise and contrast == want_contrast
    assert [(m[0, 2], m[1, 2]) for m in crops] == want_crop and out_sizes == [(8, 8)] * 5
    assert "single draw" in T.RandomCrop.__doc__.lower()


def test_random_affine_draws_twelve_seeds_up_front_in_the_stated_order():
    random.seed(3)
    cands, sizes = T.RandomAffine().draw([(20, 12), (20, 12)])
    random.seed(3)
    seeds = [[random.randint(0, 2020) for _ in range(12)] for _ in range(2)]
    assert sizes == [(20, 12)] * 2 and [len(c) for c in cands] == [12, 12]
    for k in range(2):
        for c, seed in enumerate(seeds[k]):
            rs = np.random.RandomState(seed)
            crop, scale, shear, rot = rs.uniform(0.0, 0.1, 4), rs.uniform(0.9, 1.1), rs.uniform(-15., 15.), rs.uniform(-25., 25.)
            np.testing.assert_array_equal(cands[k][c], T.affine_inverse(20, 12, crop, scale, shear, rot))


def test_resize_maps_pixel_centres_and_is_the_identity_at_equal_sizes():
    np.testing.assert_array_equal(T.resize_map(854, 480, 854, 480), np.eye(3))
    m = T.resize_map(10, 6, 20, 3)
    assert m[0, 0] == 0.5 and m[0, 2] == 0.5 * 0.5 - 0.5 and m[1, 1] == 2.0 and m[1, 2] == 0.5
    maps, sizes = T.Resize(size=(20, 3)).draw([(10, 6)])
    np.testing.assert_array_equal(maps[0], m)
    assert sizes == [(20, 3)]


def test_affine_inverse_against_a_step_by_step_composition():
    W, H, crop, scale, shear, rot = 40, 30, (0.05, 0.1, 0.0, 0.02), 1.07, 10.0, -20.0
    M = T.affine_inverse(W, H, crop, scale, shear, rot)
    cx, cy = (W - 1) / 2., (H - 1) / 2.
    th, ph = math.radians(rot), math.radians(shear)
    for x, y in ((0., 0.), (39., 29.), (12.5, 7.25), (cx, cy)):
        # forward, from a point p of the crop-resized frame: scale, shear, rotate about the centre
        px, py = 3.0 + 0.37 * x, 2.0 + 0.41 * y
        u, v = (px - cx) * scale, (py - cy) * scale
        u, v = u + math.tan(ph) * v, v
        u, v = math.cos(th) * u - math.sin(th) * v, math.sin(th) * u + math.cos(th) * v
        dx, dy = u + cx, v + cy                                             # where p lands: the inverse map must bring it back ...
        t, r, b, l = crop[0] * H, crop[1] * W, crop[2] * H, crop[3] * W
        sx = (px + 0.5) * (W - l - r) / W - 0.5 + l                         # ... and on through the crop's pixel-centre resize
        sy = (py + 0.5) * (H - t - b) / H - 0.5 + t
        got = M @ np.array([dx, dy, 1.0])
        np.testing.assert_allclose(got[:2], [sx, sy], rtol=0, atol=1e-10)
    np.testing.assert_allclose(T.affine_inverse(W, H, (0, 0, 0, 0), 1.0, 0.0, 0.0), np.eye(3), atol=1e-13)


def test_compose_hands_the_device_post_and_conjugated_candidates():
    """P A Q = (P A P^-1)(P Q): what the device composes from the rows equals the pipeline's float64 product, rounded to fp32 once."""
    random.seed(11)
    np.random.seed(11)
    pipe = T.Compose([T.Resize(size=(16, 12)), T.RandomAffine(), T.AdditiveNoise(), T.RandomContrast(), T.RandomHorizontalFlip(), T.ToTensor()])
    rows, size = pipe.draw([(20, 10), (8, 24)])
    random.seed(11)
    np.random.seed(11)
    P = [T.resize_map(20, 10, 16, 12), T.resize_map(8, 24, 16, 12)]
    A, _ = T.RandomAffine().draw([(16, 12)] * 2)
    noise, contrast = T.AdditiveNoise().draw(2), T.RandomContrast().draw(2)
    Q, _ = T.RandomHorizontalFlip().draw([(16, 12)] * 2)
    assert size == (16, 12)
    for k in range(2):
        assert rows[k]["noise"] == noise[k] and rows[k]["contrast"] == contrast[k] and len(rows[k]["cands"]) == 12
        np.testing.assert_allclose(rows[k]["post"], T._six(P[k] @ Q[k]), rtol=0, atol=1e-12)
        for c in range(12):
            full = R.compose(rows[k]["cands"][c], rows[k]["post"]).astype(np.float64)
            np.testing.assert_allclose(full, T._six(P[k] @ A[k][c] @ Q[k]), rtol=2e-6, atol=2e-5)
    with pytest.raises(ValueError, match="different sizes"):
        T.Compose([T.RandomHorizontalFlip()]).draw([(20, 10), (8, 24)])
    with pytest.raises(ValueError, match="AdditiveNoise comes before"):
        T.Compose([T.RandomContrast(), T.AdditiveNoise()])
    with pytest.raises(ValueError, match="at most one RandomAffine"):
        T.Compose([T.RandomAffine(), T.RandomAffine()])


def test_compose_of_the_restatement_is_float64_then_one_rounding():
    cand, post = (0.9, 0.1, 3.0, -0.1, 1.1, -2.0), (-1.0, 0.0, 19.0, 0.0, 1.0, 0.0)
    a, b, c, d, e, f = (float(F32(v)) for v in cand)
    want = [a * -1.0, b, (a * 19.0 + b * 0.0) + c, d * -1.0, e, (d * 19.0 + e * 0.0) + f]
    np.testing.assert_array_equal(R.compose(cand, post), np.asarray(want, np.float64).astype(F32))


def test_the_seven_names_and_signatures_of_the_reference():
    import inspect
    for name, args in (("Resize", ["scales", "size"]), ("RandomHorizontalFlip", []), ("ToTensor", []), ("RandomAffine", []),
                       ("AdditiveNoise", ["delta"]), ("RandomContrast", ["lower", "upper"]), ("RandomCrop", ["patch_size"])):
        cls = getattr(T, name)
        params = [p for p in inspect.signature(cls).parameters]
        assert params == args, name
    assert T.Resize().size == (854, 480) and T.AdditiveNoise().delta == 5.0 and T.RandomCrop().patch_size == 400
    assert (T.RandomContrast().lower, T.RandomContrast().upper) == (0.97, 1.03)
    for phrase in ("restated, not recorded", "12 seeds per frame up front", "one seed per"):
        assert phrase in T.__doc__, phrase


def test_device_samples_refuses_host_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.DeviceSamples([(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 1, 4, 4, dtype=torch.uint8))], [(0, 0, 0)])


# ------------------------------------------------------------------------------------------------ the key
def test_key_default_off_and_refusals():
    assert entry.DEFAULTS["qa_augment"] is False and entry.qa_augment_option({}) is False
    assert entry.parse_cli([]).qa_augment is False
    cfg = entry.parse_cli(["with", "setting=wild", "method=ours", "qa_report=true", "qa_augment=true"])
    assert entry.qa_augment_option(cfg) is True and entry.qa_option(cfg) == (False, True)
    with pytest.raises(SystemExit, match="qa_augment=true needs qa_report=true"):
        entry.parse_cli(["with", "qa_augment=true"])
    with pytest.raises(SystemExit, match="qa_augment=true needs qa_report=true"):
        entry.parse_cli(["with", "setting=wild", "method=ours", "qa_report=false", "qa_augment=true"])
    for bad in ("1", "yes", "none", "2.5"):
        with pytest.raises(SystemExit, match="qa_augment must be true or false"):
            entry.parse_cli(["with", f"qa_augment={bad}"])
    cfg = entry.parse_cli(["with", "synthetic=1"])
    cfg.qa_augment = True                                                    # run_eval refuses before any work
    with pytest.raises(ValueError, match="qa_augment"):
        entry.run_eval(cfg)


def test_the_loop_prints_the_aug_line_only_under_true(monkeypatch, tmp_path, capsys, host_quantiser):  # noqa: F811
    loop = _Loop(monkeypatch, tmp_path)
    monkeypatch.setattr(utils_agent, "assess_report", lambda videos, scores, metric: (np.asarray([[0.25, 0.5, 3]], np.float32), None))
    calls = []

    def restated(videos, assess_net, metric, transform=None, seed=None, **kw):
        """The device chain's stand-in: the draws of the train transform and the numpy restatement of the warp; the measures are the
        share of units whose augmented label or mask is not empty (no AssessNet on the CPU)."""
        (frames, gt, planes, n_objects), = videos
        frames, gt, planes = (np.ascontiguousarray(np.asarray(t)) for t in (frames, gt, planes))
        n, H, W = gt.shape
        samples = [dict(v=0, f=f, o=o) for o in range(n_objects) for f in range(n)]
        state = random.getstate(), np.random.get_state()
        random.seed(seed)
        np.random.seed(seed)
        rows, (Wo, Ho) = T.train_transform(size=(W, H)).draw([(W, H)] * len(samples))
        random.setstate(state[0])
        np.random.set_state(state[1])
        out = R.augment([dict(frames=frames.astype(F32), gt=gt, planes=planes, obj_ids=list(range(1, n_objects + 1)))],
                        [dict(s, **r) for s, r in zip(samples, rows)], Ho, Wo)
        valid = int(((out["label"] > 0) | (out["mask"] > 0)).reshape(len(samples), -1).any(1).sum())
        calls.append((seed, len(samples), out["chosen"].tolist()))
        return np.asarray([[0.125, 0.375, valid]], np.float32), None
    monkeypatch.setattr(utils_agent, "assess_report_augmented", restated)
    _, calls_off, sum_off = loop.run("off", ["qa_report=true", "qa_augment=false"])
    text_off = capsys.readouterr().out
    assert calls == [] and " aug " not in text_off and "qa_augment" not in text_off and "augmented" not in sum_off.decode()
    _, calls_absent, sum_absent = loop.run("absent", ["qa_report=true"])
    text_absent = capsys.readouterr().out
    strip = lambda t, k: re.sub(r"(rec_time:|recommend_frame avg )\s*[0-9.]+", r"\1T", t.replace(f"{tmp_path}/{k}", "DIR"))   # noqa: E731
    assert strip(text_absent, "absent") == strip(text_off, "off") and sum_absent == sum_off and calls_absent == calls_off
    _, calls_on, sum_on = loop.run("on", ["qa_report=true", "qa_augment=true"])
    text_on = capsys.readouterr().out
    assert calls_on == calls_off                                             # the loop's own calls are untouched
    assert len(calls) == 4 and [c[0] for c in calls] == [entry.DEFAULTS["seed"] + i for i in range(4)]
    assert all(len(ch) == n and all(0 <= c <= 12 for c in ch) for _, n, ch in calls)
    lines = [ln for ln in text_on.splitlines() if ln.startswith("avg_")]
    assert len(lines) == 4 and all(re.search(r"valid: 3/\d+ aug loss 0\.1250 diff 0\.3750 n \d+ ", ln) for ln in lines)
    assert [strip(re.sub(r"aug loss .* n \d+ ", "", ln), "on") for ln in lines] == \
        [strip(ln, "off") for ln in text_off.splitlines() if ln.startswith("avg_")]
    on, off = json.loads(sum_on), json.loads(sum_off)
    assert set(on["qa"]["augmented"]) == {"loss", "diff", "valid"} and on["qa"]["augmented"]["loss"] == 0.125
    assert {k: v for k, v in on["qa"].items() if k != "augmented"} == off["qa"]
    assert {k: v for k, v in on.items() if k != "qa"} == {k: v for k, v in off.items() if k != "qa"}


# ------------------------------------------------------------------------------------------------ header, bindings, build
def test_header_bindings_and_build_agree():
    header = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for name in ("ivosw_qa_augment_ws_bytes", "ivosw_qa_augment"):
        assert name in L.SIGNATURES and name + "(" in header
    for phrase in ("THE SAMPLING RULE", "sx = fl(fl(fl(a*x) + fl(b*y)) + c)", "top = v00 + fx * (v10 - v00)", "floor(sx + 0.5f)",
                   "float32(b) / 255.0f", "clip(fl(v + noise), 0, 1)", "prob > 0.8f", "One destination pixel per lane", "datasets/transforms_assess.py"):
        assert phrase in header, phrase
    from ivos_w_amd import build
    assert "qa_augment.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "qa_augment.hip"))
    assert ctypes.sizeof(L.AugSample) == 4 * (4 + 72 + 6 + 2) and L.AugSample.post.offset == 16 + 288
    assert ctypes.sizeof(L.AugVideo) == 80 and L.AugVideo.obj_ids.offset == 44
    assert "IVOSW_AUGMENT_SCALAR" not in header + open(os.path.join(build.CSRC, "qa_augment.hip")).read()      # one path, no switch
    assert L.QA_AUG_MAX_CAND == 12 == R.MAX_CAND and "#define IVOSW_QA_AUG_MAX_CAND 12" in header
    for doc in ("README.md", "DESIGN.md", "SURVEY.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ivosw_qa_augment" in text and "transforms_assess" in text, doc
