"""CPU: the overlay rules as tests/overlay_ref.py restates them against the pictures recorded from the reference
(tests/golden/overlay_fixtures.npz), the palette, the overlay / overlay_frames keys of the entry scripts, and what the wrappers of
utils/utils_ipn.py refuse before they touch the GPU."""
import os

import numpy as np
import pytest

from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.utils import utils_ipn
from tests import overlay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "overlay_fixtures.npz")


def test_the_restatement_equals_every_recorded_picture():
    g = np.load(GOLD)
    assert [tuple(s) for s in g["sizes"]] == [(9, 33), (33, 70)] and int(g["n_objects"]) == 3
    seen = set()
    for H, W in g["sizes"]:
        key = f"{H}x{W}_"
        img, lab = g[key + "image"], g[key + "label"]
        assert img.dtype == np.uint8 and img.shape == (H, W, 3) and lab.shape == (H, W) and lab.max() > 3
        assert {int(lab[0, 0]), int(lab[0, W - 1]), int(lab[H - 1, 0]), int(lab[H - 1, W - 1])} == {1, 2, 3}      # every corner
        cases = {"fade": ("fade", 1, dict(select=1)), "checker": ("checker", 3, dict(select=1)), "color": ("color", 3, dict(select=1)),
                 "color_rgb": ("color", 3, dict(select=1, color=(3, 250, 9)))}
        for a in (0.5, 0.3):
            cases[f"davis_a{a}"] = ("davis", 1, dict(select=1, alpha=a, palette=[(255, 0, 0)]))
            cases[f"davis_rgb_a{a}"] = ("davis", 3, dict(select=1, alpha=a, palette=[(10, 201, 77)]))
            cases[f"davis_seq_a{a}"] = ("davis", 3, dict(select=0, alpha=a))                                     # three objects, in sequence
            cases[f"davis_obj2_a{a}"] = ("davis", 3, dict(select=2, alpha=a))
        for name, (style, n_objects, kw) in cases.items():
            np.testing.assert_array_equal(R.overlay_one(img, lab, style, n_objects, **kw), g[key + name], err_msg=key + name)
            seen.add(key + name)
        # the sequential composition differs from every single-object picture, and a touching pair shows both rules of the walk
        assert not np.array_equal(g[key + "davis_seq_a0.5"], g[key + "davis_obj2_a0.5"])
        seq = g[key + "davis_seq_a0.5"]
        y, x = 0, W // 3                                                  # object 2 right of object 1 in row 0
        assert lab[y, x - 1] == 1 and lab[y, x] == 2
        assert tuple(seq[y, x - 1]) == (0, 0, 0) and tuple(seq[y, x]) == (0, 64, 0)                                # 0, and trunc(0 * alpha + k2)
    assert seen == {k for k in g.files if k[0].isdigit() and not k.endswith(("image", "label"))}               # no recorded picture is left out


def test_palette_and_frame_bytes():
    pal = utils_ipn.davis_palette()
    assert pal.dtype == np.uint8 and pal.shape == (32, 3)
    assert [tuple(int(v) for v in r) for r in pal[:4]] == [(128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128)]
    assert tuple(int(v) for v in pal[7]) == (64, 0, 0) and tuple(int(v) for v in pal[31]) == (0, 0, 64)           # objects 8 and 32
    assert len({tuple(r) for r in pal}) == 32 and not (pal == 0).all(1).any()
    np.testing.assert_array_equal(pal, R.davis_palette())
    np.testing.assert_array_equal(np.load(GOLD)["palette3"], pal[:3])
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1).repeat(3, 3)
    f = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    np.testing.assert_array_equal(R.frame_bytes(f), u8)                                                          # u8 / 255 gives u8 back
    odd = np.array([np.nan, -1.0, -1e-9, 2.0, np.inf, -np.inf, 0.6 / 255, 0.4 / 255], np.float32).reshape(1, 1, 1, 8).repeat(3, 1)
    assert R.frame_bytes(odd)[0, 0, :, 0].tolist() == [0, 0, 0, 255, 255, 0, 1, 0]


def test_overlay_options_struct():
    o = utils_ipn.overlay_options("fade", 3, 2, 0.25, [(1, 2, 3), (4, 5, 6)], (7, 8, 9))
    assert isinstance(o, L.Overlay) and (o.style, o.n_objects, o.select, o.alpha) == (L.OVERLAY_FADE, 3, 2, 0.25)
    assert [list(r) for r in o.palette][:3] == [[1, 2, 3], [4, 5, 6], [0, 0, 0]] and list(o.color) == [7, 8, 9]
    assert [list(r) for r in utils_ipn.overlay_options("davis", 32).palette] == utils_ipn.davis_palette().tolist()
    assert [utils_ipn.OVERLAY_STYLES[s] for s in R.STYLES] == [0, 1, 2, 3]
    for bad in (dict(style="glow"), dict(style=0), dict(n_objects=0), dict(n_objects=33), dict(select=-1), dict(select=4), dict(alpha=-0.1),
                dict(alpha=1.1), dict(alpha=float("nan")), dict(palette=[(1, 2)]), dict(palette=np.zeros((33, 3))), dict(color=(1, 2))):
        with pytest.raises(ValueError):
            utils_ipn.overlay_options(**dict(dict(style="davis", n_objects=3), **bad))


def test_overlay_option_accepts_and_refuses():
    assert entry.DEFAULTS["overlay"] == "none" and entry.DEFAULTS["overlay_frames"] == "candidates"
    assert entry.overlay_option({}) == ("none", "candidates")
    cfg = entry.parse_cli([])
    assert (cfg.overlay, cfg.overlay_frames) == ("none", "candidates")
    for style in ("none", "davis", "fade", "checker", "color"):
        for which in ("candidates", "all"):
            cfg = entry.parse_cli(["with", f"overlay={style}", f"overlay_frames={which}"])
            assert (cfg.overlay, cfg.overlay_frames) == (style, which) == entry.overlay_option(cfg)
    for bad in ("Davis", "glow", "1", "true", "", "all"):
        with pytest.raises(SystemExit, match="overlay must be"):
            entry.parse_cli(["with", f"overlay={bad}"])
    for bad in ("none", "All", "candidate", "3", ""):
        with pytest.raises(SystemExit, match="overlay_frames must be"):
            entry.parse_cli(["with", "overlay=davis", f"overlay_frames={bad}"])
    for bad in (1, True, ("davis",)):
        with pytest.raises(SystemExit, match="overlay"):
            entry.parse_cli([], overlay=bad)
    with pytest.raises(ValueError, match="overlay must be 'none', 'davis', 'fade', 'checker' or 'color', got 'glow'"):
        entry.overlay_option(dict(overlay="glow"))
    with pytest.raises(ValueError, match="overlay_frames must be 'candidates' or 'all', got 'some'"):
        entry.overlay_option(dict(overlay="fade", overlay_frames="some"))
    cfg = entry.parse_cli(["with", "synthetic=1"])                       # run_eval refuses a bad value before any work
    cfg.overlay = "glow"
    with pytest.raises(ValueError, match="overlay"):
        entry.run_eval(cfg)


def test_write_image_round_trip(tmp_path):
    rgb = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = entry.write_image(str(tmp_path / "00003"), rgb)
    if path.endswith(".png"):
        from PIL import Image
        back = np.asarray(Image.open(path).convert("RGB"))
    else:
        raw = open(path, "rb").read()
        assert path.endswith(".ppm") and raw.startswith(b"P6\n7 5\n255\n")
        back = np.frombuffer(raw[len(b"P6\n7 5\n255\n"):], np.uint8).reshape(5, 7, 3)
    np.testing.assert_array_equal(back, rgb)


def test_wrappers_refuse_before_touching_the_gpu(monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the library was reached"))
    img, mask = np.zeros((4, 6, 3), np.uint8), np.ones((4, 6))
    for fn in (utils_ipn.overlay_davis, utils_ipn.overlay_fade, utils_ipn.overlay_checker, utils_ipn.overlay_color):
        for bad in (img.astype(np.float32), img.astype(np.float64) / 255, img.astype(np.int32), img.astype(bool)):
            with pytest.raises(TypeError, match="uint8 image"):
                fn(bad, mask)
        with pytest.raises(ValueError):
            fn(img[..., :2], mask)
        with pytest.raises(ValueError):
            fn(img, mask[:3])
    with pytest.raises(ValueError, match="alpha"):
        utils_ipn.overlay_davis(img, mask, alpha=2.0)
    import torch
    with pytest.raises((TypeError, RuntimeError)):
        utils_ipn.overlay_session(torch.zeros(2, 3, 4, 6), torch.zeros(2, 4, 6, dtype=torch.uint8), 3)       # host tensors: no CPU fallback
    with pytest.raises(ValueError, match="style"):
        utils_ipn.overlay_session(torch.zeros(2, 3, 4, 6), torch.zeros(2, 4, 6, dtype=torch.uint8), 3, style="glow")


def test_header_cites_the_reference_and_the_build_lists_the_source():
    header = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    for cite in (":113-128", ":131-143", ":146-157", ":160-171", ":174-190", "simply continues"):
        assert cite in header, cite
    from ivos_w_amd import build
    assert "overlay.hip" in build.SOURCES and "ivosw_overlay_frames" in L.SIGNATURES and "ivosw_overlay_lane_pixels" in L.SIGNATURES


def test_lane_pixels_rule():
    """Host only: the widest of 4, 2, 1 pixels per lane whose words all lie on their grids; W = 854 (DAVIS 480p) takes 2."""
    import ctypes
    lib = L.lib()
    q = lambda fr, lab, W, out, kind: lib.ivosw_overlay_lane_pixels(ctypes.c_void_p(fr), ctypes.c_void_p(lab), W, ctypes.c_void_p(out), kind)
    base = 1 << 20
    for kind in (L.OUT_RGB8, L.OUT_RGBX8):
        assert [q(base, base, W, base, kind) for W in (856, 854, 853, 64, 70, 2, 1, 4)] == [4, 2, 1, 4, 2, 2, 1, 4]
        assert q(base + 8, base, 856, base, kind) == 2 and q(base + 4, base, 856, base, kind) == 1 and q(base + 16, base, 856, base, kind) == 4
        assert q(base, base + 2, 856, base, kind) == 2 and q(base, base + 1, 856, base, kind) == 1
    assert [q(base, base, 856, base + o, L.OUT_RGB8) for o in (1, 2, 3, 4, 6)] == [1, 2, 1, 4, 2]
    assert [q(base, base, 856, base + o, L.OUT_RGBX8) for o in (4, 8, 12, 16)] == [1, 2, 1, 4]
