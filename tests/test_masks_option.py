"""masks=labels without a GPU: the option parser and its refusal, the LabelMasks holder (shape and dtype checks, from_probs against
numpy's argmax with ties, to_planes), ScoreCache's byte count and key for both mask kinds, the header / binding / SIGNATURES agreement
of the seven *_lab entries, and the *_lab refusals that are issued before any pointer is used."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models.assessment import MASK_KINDS, AssessNet, LabelMasks, ScoreCache
from ivos_w_amd.utils import utils_agent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAB_ENTRIES = ("ivosw_mask_bbox_videos", "ivosw_roi_sample_videos", "ivosw_assess_forward_videos", "ivosw_mask_delta_videos",
               "ivosw_mask_bbox_units", "ivosw_roi_sample_units", "ivosw_assess_forward_units")


# ---------------------------------------------------------------------------------------------- the option
def test_masks_option_and_its_refusal():
    assert entry.MASK_MODES == ("float32", "labels") == MASK_KINDS
    assert entry.DEFAULTS["masks"] == "float32"
    assert entry.parse_cli([]).masks == "float32"
    assert entry.parse_cli(["with", "masks=labels"]).masks == "labels"
    assert entry.parse_cli(["with", "masks=labels", "frames=uint8", "rescore=changed", "precision=bf16"]).masks == "labels"
    for bad in ("uint8", "label", "Labels", "float", "", "1"):
        with pytest.raises(SystemExit, match="masks must be 'float32' or 'labels'"):
            entry.parse_cli(["with", f"masks={bad}"])
    for bad in (1, None, True, ("labels",)):
        with pytest.raises(SystemExit, match="masks"):
            entry.parse_cli([], masks=bad)
    # read with .get: a config written before the key existed keeps float masks; run_eval refuses a bad value before any work
    assert entry.masks_option({}) == "float32" and entry.masks_option(dict(masks="labels")) == "labels"
    with pytest.raises(ValueError, match="masks must be 'float32' or 'labels', got 'soft'"):
        entry.masks_option(dict(masks="soft"))
    cfg = entry.parse_cli(["with", "synthetic=1"])
    cfg.masks = "bytes"
    with pytest.raises(ValueError, match="masks"):
        entry.run_eval(cfg)
    # the other options are untouched
    assert entry.parse_cli([]).frames == "float32" and entry.parse_cli([]).rescore == "all"


def test_harden_hands_on_or_hardens():
    P = torch.rand(2, 3, 4, 5)
    assert entry._harden(P, "float32") is P
    lab = entry._harden(P, "labels")
    assert isinstance(lab, LabelMasks) and torch.equal(lab.map, P.argmax(1).to(torch.uint8))


# ---------------------------------------------------------------------------------------------- LabelMasks
def test_label_masks_shape_and_dtype_checks():
    ok = torch.zeros(3, 5, 7, dtype=torch.uint8)
    m = LabelMasks(ok)
    assert (m.n, m.H, m.W, len(m)) == (3, 5, 7, 3) and m.device == ok.device and m.map is ok and not m.is_cuda
    assert m.to("cpu") is m
    for bad in (ok.float(), ok.to(torch.int8), ok.to(torch.int64), ok.bool(), ok.numpy(), None, [[[1]]]):
        with pytest.raises(TypeError, match="uint8"):
            LabelMasks(bad)
    for bad in (ok[0], ok[None], torch.zeros(0, 5, 7, dtype=torch.uint8), torch.zeros(2, 0, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[n,H,W\]"):
            LabelMasks(bad)
    # the two last dimensions are made contiguous; a frame stride above H * W is kept (no copy)
    t = torch.arange(3 * 7 * 5, dtype=torch.uint8).view(3, 7, 5).permute(0, 2, 1)
    c = LabelMasks(t)
    assert c.map.is_contiguous() and torch.equal(c.map, t)
    wide = torch.zeros(3, 50, dtype=torch.uint8)[:, :35].view(3, 5, 7)
    assert wide.stride(0) == 50 and LabelMasks(wide).map is wide
    cropped = torch.zeros(3, 5, 9, dtype=torch.uint8)[:, :, :7]
    assert LabelMasks(cropped).map.is_contiguous()
    expanded = torch.zeros(1, 5, 7, dtype=torch.uint8).expand(3, 5, 7)           # frames that overlap: copied apart
    assert LabelMasks(expanded).map.stride(0) == 35


def test_from_probs_is_numpys_argmax_ties_included():
    g = torch.Generator().manual_seed(5)
    P = torch.rand(3, 4, 6, 9, generator=g)
    P[0, :, 0, 0] = 0.5                                                          # a four-way tie: the first maximum, the background
    P[0, 1:, 0, 1] = 0.9                                                         # objects 1 .. 3 tie above the background: object 1
    P[1, 2:, 2, 2] = 1.0                                                         # objects 2, 3 tie: object 2
    P[2, :, 5, 8] = 0.0
    lab = LabelMasks.from_probs(P)
    assert lab.map.dtype == torch.uint8 and tuple(lab.map.shape) == (3, 6, 9)
    np.testing.assert_array_equal(lab.map.numpy(), np.argmax(P.numpy(), axis=1).astype(np.uint8))
    assert [int(lab.map[0, 0, 0]), int(lab.map[0, 0, 1]), int(lab.map[1, 2, 2]), int(lab.map[2, 5, 8])] == [0, 1, 2, 0]
    # any layout all_P comes in (the object-major ProbStore view)
    Pv = P.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert torch.equal(LabelMasks.from_probs(Pv).map, lab.map)
    for bad in (P[0], P.numpy(), None):
        with pytest.raises(ValueError, match="all_P"):
            LabelMasks.from_probs(bad)
    with pytest.raises(ValueError, match="255"):
        LabelMasks.from_probs(torch.zeros(1, 257, 2, 2))
    assert "DISCARDS" in LabelMasks.from_probs.__doc__                           # the docstring says what is lost


def test_to_planes_is_the_one_hot_definition():
    m = torch.tensor([[[0, 1, 2], [3, 4, 255]], [[2, 2, 0], [1, 1, 1]]], dtype=torch.uint8)
    lab = LabelMasks(m)
    for O in (1, 3):
        planes = lab.to_planes(O)
        assert planes.dtype == torch.float32 and tuple(planes.shape) == (2, O + 1, 2, 3)
        for o in range(O):
            assert torch.equal(planes[:, o + 1], (m == o + 1).float())           # tp = (map == obj + 1) ? 1.0f : 0.0f
        assert torch.equal(planes[:, 0], ((m == 0) | (m > O)).float())           # label 0 and labels above n_obj: no object
        assert torch.equal(planes.sum(1), torch.ones(2, 2, 3))
    # hard labels survive the round trip when every label is an object's
    inside = LabelMasks(m.clamp(max=3))
    assert torch.equal(LabelMasks.from_probs(inside.to_planes(3)).map, inside.map)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="n_obj"):
            lab.to_planes(bad)


# ---------------------------------------------------------------------------------------------- the score cache
def test_score_cache_bytes_and_key_for_both_kinds():
    n, O, H, W = 100, 3, 480, 854
    f32 = ScoreCache.nbytes_for(n, O, H, W)
    assert f32 == ScoreCache.nbytes_for(n, O, H, W, "float32") == 4 * n * O * (H * W + 1)     # the planes and the score table
    lab = ScoreCache.nbytes_for(n, O, H, W, masks="labels")
    assert lab == n * H * W + 4 * n * O                                                         # ONE uint8 map per frame and the table
    assert 0.49e9 < f32 < 0.5e9 and 40.9e6 < lab < 41.1e6 and f32 // lab == 11
    assert ScoreCache.nbytes_for(2, 255, 3, 5, "labels") == 2 * 15 + 4 * 2 * 255
    with pytest.raises(ValueError, match="masks"):
        ScoreCache.nbytes_for(1, 1, 2, 2, "uint8")
    net, frames = AssessNet(precision="bf16"), torch.zeros(2, 3, 4, 6)
    kf, src = ScoreCache.make_key(net, frames, 2, 1, 4, 6)
    kl, _ = ScoreCache.make_key(net, frames, 2, 1, 4, 6, "labels")
    assert src is frames and kf != kl and kf[:8] == kl[:8] and (kf[8], kl[8]) == ("float32", "labels")
    assert kf == ScoreCache.make_key(net, frames, 2, 1, 4, 6, "float32")[0]
    with pytest.raises(ValueError, match="masks"):
        ScoreCache.make_key(net, frames, 2, 1, 4, 6, "soft")
    # bind: the copy of the masks in the session's format; switching kinds makes the cache cold and reallocates
    c = ScoreCache()
    assert c.nbytes == 0
    assert c.bind(net, frames, 2, 3, 4, 6, "cpu", masks="labels") is True
    assert c.planes.dtype == torch.uint8 and c.planes.numel() == 2 * 24 and tuple(c.scores.shape) == (3, 2) and c.units == 6
    assert c.nbytes == ScoreCache.nbytes_for(2, 3, 4, 6, "labels") == c.planes.numel() + 4 * c.scores.numel()
    assert c.bind(net, frames, 2, 3, 4, 6, "cpu", masks="labels") is False                      # warm
    assert c.bind(net, frames, 2, 3, 4, 6, "cpu") is True                                       # the other kind: cold
    assert c.planes.dtype == torch.float32 and c.planes.numel() == 3 * 2 * 24
    assert c.nbytes == ScoreCache.nbytes_for(2, 3, 4, 6) == 4 * (c.planes.numel() + c.scores.numel())
    assert c.bind(net, frames, 2, 3, 4, 6, "cpu") is False
    assert c.bind(net, frames, 2, 3, 4, 6, "cpu", masks="labels") is True


def test_the_lru_accounts_the_real_bytes():
    net, frames = AssessNet(precision="bf16"), torch.zeros(5, 3, 8, 10)
    lab = LabelMasks(torch.zeros(5, 8, 10, dtype=torch.uint8))
    lru = utils_agent._ScoreCacheLRU()
    a, = lru.get_many(net, [(frames, None, 2)])
    assert lru.nbytes() == ScoreCache.nbytes_for(5, 2, 8, 10)
    b, = lru.get_many(net, [(frames, lab, 2)])                                  # the same frames with label masks: another entry
    assert b is not a and lru.nbytes() == ScoreCache.nbytes_for(5, 2, 8, 10) + ScoreCache.nbytes_for(5, 2, 8, 10, "labels")
    assert lru.get_many(net, [(frames, lab, 2)])[0] is b and lru.get_many(net, [(frames, None, 2)])[0] is a
    lru.trim(ScoreCache.nbytes_for(5, 2, 8, 10))                                # room for the float entry only: the older label entry goes
    assert list(e[0] for e in lru.entries.values()) == [a]


def test_masks_on_uploads_only_what_is_elsewhere():
    lab = LabelMasks(torch.zeros(2, 3, 4, dtype=torch.uint8))
    assert utils_agent._masks_on(lab, "cpu") is lab and utils_agent._is_labels(lab)
    P = torch.zeros(2, 2, 3, 4)
    assert not utils_agent._is_labels(P) and not utils_agent._is_labels(lab.map)  # only the type selects the path


# ---------------------------------------------------------------------------------------------- C ABI
def test_header_binding_and_signatures_agree():
    S = L.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    assert "typedef struct ivosw_labels { const uint8_t* map; long stride_frame; } ivosw_labels_t;" in " ".join(
        hdr.replace("/* device; NULL: a float video */", "").replace("/* elements */", "").split())
    assert [f[0] for f in L.Labels._fields_] == ["map", "stride_frame"]
    assert ctypes.sizeof(L.Labels) == 16 and L.Labels.stride_frame.offset == 8
    flat = " ".join(hdr.split())
    for name in LAB_ENTRIES:
        res, args = S[name]
        lres, largs = S[name + "_lab"]
        v = 2 if name.startswith("ivosw_assess_forward") else 0                   # `videos`: behind (packed, dtype) in the forward entries
        assert lres is res and largs == args[:v + 1] + [L._p] + args[v + 1:], name  # `labels` right after `videos`, nothing else
        plain = flat[flat.index(f"int {name}("):]
        plain = plain[:plain.index(");")]
        lab = flat[flat.index(f"int {name}_lab("):]
        lab = lab[:lab.index(");")]
        want = plain.replace(f"{name}(", f"{name}_lab(").replace("const ivosw_video_t* videos,", "const ivosw_video_t* videos, const ivosw_labels_t* labels,")
        if name == "ivosw_mask_delta_videos":                                     # the cache of a label video is uint8: untyped pointers
            want = want.replace("float* const* cache", "void* const* cache")
        assert lab == want, name
        assert lab.count(",") + 1 == len(largs), name
    # ivosw_video_t keeps its layout
    assert [f[0] for f in L.Video._fields_] == ["frames", "masks", "mask_stride_frame", "mask_stride_obj", "frames_kind", "n_frames", "n_obj",
                                                "H", "W"] and ctypes.sizeof(L.Video) == 56
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "LabelMasks" in text and "masks=labels" in text, doc


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _fake():
    """A non-NULL host pointer that must never be dereferenced: every case below is refused before any pointer is used."""
    buf = ctypes.create_string_buffer(96)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def _calls(lib, p):
    """name -> call(videos, labels, n_videos) of the seven *_lab entries with harmless other arguments."""
    P = ctypes.c_void_p(p)
    return {
        "ivosw_mask_bbox_videos_lab": lambda v, l, n: lib.ivosw_mask_bbox_videos_lab(v, l, n, P, P, None),
        "ivosw_roi_sample_videos_lab": lambda v, l, n: lib.ivosw_roi_sample_videos_lab(v, l, n, P, L.BF16, P, None),
        "ivosw_assess_forward_videos_lab": lambda v, l, n: lib.ivosw_assess_forward_videos_lab(P, L.BF16, v, l, n, P, P, 1 << 20, 0, 0, None, None),
        "ivosw_mask_delta_videos_lab": lambda v, l, n: lib.ivosw_mask_delta_videos_lab(v, l, n, (ctypes.c_void_p * 2)(p, p), L.int_array([0, 0]),
                                                                                      P, P, P, None),
        "ivosw_mask_bbox_units_lab": lambda v, l, n: lib.ivosw_mask_bbox_units_lab(v, l, n, P, 1, P, P, None),
        "ivosw_roi_sample_units_lab": lambda v, l, n: lib.ivosw_roi_sample_units_lab(v, l, n, P, 1, P, L.BF16, P, None),
        "ivosw_assess_forward_units_lab": lambda v, l, n: lib.ivosw_assess_forward_units_lab(P, L.BF16, v, l, n, P, 1, P, P, 1 << 20, 0, None),
    }


def test_lab_entries_refuse_before_any_launch(lib):
    keep, p = _fake()
    msg = lambda: lib.ivosw_last_error().decode()
    video = lambda masks=None, n=2, O=2, H=8, W=8: L.Video(p, masks, H * W, n * H * W, L.FRAMES_F32, n, O, H, W)
    for name, call in _calls(lib, p).items():
        labels = (L.Labels * 2)(L.Labels(p, 64), L.Labels(None, 0))
        # a NULL table; n_videos out of range
        assert call(None, labels, 2) == -1 and "null pointer (videos)" in msg() and name in msg(), name
        assert call((L.Video * 2)(video(), video(p)), labels, 0) == -1 and "n_videos" in msg(), name
        # n_obj = 256 on a label video (255 passes this check and goes on to the device-pointer check); a float video may hold more
        assert call((L.Video * 2)(video(O=256), video(p)), labels, 2) == -1 and "video 0" in msg() and "255" in msg(), name
        assert call((L.Video * 2)(video(O=255), video(p, O=256)), labels, 2) == -1 and "255" not in msg(), name
        # the label stride: negative; frames that overlap (fine with one frame)
        bad = (L.Labels * 2)(L.Labels(p, -64), L.Labels(None, 0))
        assert call((L.Video * 2)(video(), video(p)), bad, 2) == -1 and "video 0" in msg() and "negative" in msg(), name
        bad = (L.Labels * 2)(L.Labels(p, 63), L.Labels(None, 0))
        assert call((L.Video * 2)(video(), video(p)), bad, 2) == -1 and "video 0" in msg() and "overlap" in msg(), name
        assert call((L.Video * 2)(video(n=1), video(p)), bad, 2) == -1 and "overlap" not in msg(), name
        # a float video with NULL masks - in a mixed table and with labels == NULL (the plain entry's refusal)
        assert call((L.Video * 2)(video(), video(None)), labels, 2) == -1 and "video 1" in msg() and "null pointer" in msg(), name
        assert call((L.Video * 2)(video(None), video(p)), None, 2) == -1 and "video 0" in msg() and "null pointer" in msg(), name
        # the plain entry's refusals stand for a label video too
        assert call((L.Video * 2)(video(H=1), video(p)), labels, 2) == -1 and "video 0" in msg() and "H, W > 1" in msg(), name


def test_new_kernels_have_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    table = kr.kernel_table(L.LIB_PATH)
    for key, count in (("bbox_scan_multi_kernel", 4), ("roi_sample_multi_kernel", 8), ("mask_delta_kernel", 2), ("mask_delta_lab_kernel", 1)):
        hits = [r for n, r in table.items() if key in n]
        assert len(hits) == count, (key, len(hits))
        assert all(r["spill"] == 0 and r["scratch"] == 0 for r in hits), (key, hits)
