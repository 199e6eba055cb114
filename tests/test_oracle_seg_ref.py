"""CPU: the float64 reference of the segmentation epilogue (oracle/seg_ref.py) and the inputs of tests/test_gpu_seg_edges.py.
  * the reference's coordinate convention is ATen's: torch's float32 interpolate lies within the derived bound 7 * 2^-24 * M of it
    on every case (a different source index would miss by a whole logit difference, ~1e6 bounds)
  * so does a plain float32 evaluation in the kernel's order of operations
  * every chosen input keeps its near-ties (float64 top-two gap <= twice the bound) under the cap of 1e-3, by the reference alone
  * the case table names the kernel instantiation each case runs, and together they run all ten."""
import numpy as np
import pytest
import torch

from oracle import seg_ref as sr


@pytest.fixture(scope="module")
def refs():
    return {}


def _ref(refs, c):
    if c.name not in refs:
        x = sr.case_logits(c)
        refs[c.name] = (x, sr.reference(x, c.H, c.W))
    return refs[c.name]


@pytest.mark.parametrize("c", sr.CASES, ids=lambda c: c.name)
def test_torch_fp32_and_the_fp32_model_lie_within_the_bound(refs, c):
    x, ref = _ref(refs, c)
    assert x.dtype == np.float32 and ref.up.shape == (c.k, c.C, c.H, c.W)
    up_t, p_t = sr.torch_fp32(x, c.H, c.W)
    for name, up in (("torch", up_t), ("model", sr.upsample_f32_model(x, c.H, c.W))):
        ratio = np.abs(up.astype(np.float64) - ref.up) / np.maximum(ref.bound, 1e-300)
        assert ratio.max() <= 1.0, (name, ratio.max())
    # labels of torch itself pass the label check, and its probabilities are close: the reference computes the same operation
    sr.check_labels(up_t.argmax(1), ref)
    assert np.abs(p_t - ref.probs).max() < 1e-4


@pytest.mark.parametrize("c", sr.CASES, ids=lambda c: c.name)
def test_near_ties_stay_under_the_cap(refs, c):
    _, ref = _ref(refs, c)
    assert ref.near_tie.mean() <= sr.NEAR_TIE_CAP, ref.near_tie.mean()
    assert (ref.gap >= 0).all() and ((ref.label != ref.second) | (c.C == 1)).all()


def test_c256_input_has_class_255_on_top():
    x = sr.logits_256()
    ref = sr.reference(x, 6, 10)
    assert ref.near_tie.mean() <= sr.NEAR_TIE_CAP
    labels = set(np.unique(ref.label).tolist())
    assert {0, 128, 255} <= labels and ref.label[0, 5, 9] == 255
    up_t, _ = sr.torch_fp32(x, 6, 10)
    assert (np.abs(up_t - ref.up) <= ref.bound).all()


def test_case_table_runs_every_instantiation():
    for c in sr.CASES:
        assert sr.expected_kernel(c.C, c.H, c.W) == c.kernel, c.name
        assert c.H * c.W <= 130 * 130
    assert {c.kernel for c in sr.CASES} == {f"<{cm},{v}>" for cm in (4, 8, 16) for v in ("4,full", "4", "1")} | {"generic"}
    by = lambda f: [c for c in sr.CASES if f(c)]                     # noqa: E731
    assert {c.C for c in by(lambda c: c.kernel.endswith("full>"))} >= {4, 8, 16}
    assert {c.C for c in by(lambda c: c.kernel.endswith(",4>"))} >= {3, 5, 11}
    assert {c.C for c in by(lambda c: c.kernel.endswith(",1>"))} >= {3, 6, 13}
    assert {c.C for c in by(lambda c: c.kernel == "generic")} >= {17, 20}
    assert {c.W % 4 for c in by(lambda c: ",4" in c.kernel)} == {0, 1, 2, 3}          # V = 4 threads that straddle a row end
    assert by(lambda c: c.H < c.hs and c.W < c.ws) and by(lambda c: c.H < c.hs and c.W > c.ws) and by(lambda c: c.H > c.hs and c.W < c.ws)
    assert by(lambda c: c.H == 1 and c.W > 1) and by(lambda c: c.H > 1 and c.W == 1) and by(lambda c: c.hs == 1 and c.ws > 1)
    assert by(lambda c: (c.H, c.W) == (c.hs, c.ws)) and by(lambda c: c.ws >= 300 and c.W >= 1200 and c.H == 4)
    assert {c.variant for c in sr.CASES} == {"plain", "offset", "wide"}


def test_wide_variant_underflows_and_offset_variant_is_large():
    for c in sr.CASES:
        x, ref = sr.case_logits(c), None
        if c.variant == "wide":
            ref = sr.reference(x, c.H, c.W)
            assert (ref.probs < 2.0 ** -149).any() and np.abs(x).max() > 40          # below float32's smallest subnormal
        if c.variant == "offset":
            assert x.min() > 80


def test_older_bar_against_torch_has_no_meaning_on_the_variants():
    """The older GPU test holds the kernel to 2e-6 absolute of torch's float32 probabilities.  On the offset and wide variants torch's own
    error against float64 already is of that size, and a faithful float32 evaluation in another order of operations lies further than
    2e-6 from torch: the GPU test keeps that bar on the plain inputs and uses the comparison against float64 on the variants."""
    worst_plain, apart = 0.0, []
    for c in sr.CASES:
        x, ref = sr.case_logits(c), sr.reference(sr.case_logits(c), c.H, c.W)
        p_t = sr.torch_fp32(x, c.H, c.W)[1]
        p_m = torch.softmax(torch.from_numpy(sr.upsample_f32_model(x, c.H, c.W)), 1).numpy()
        if c.variant == "plain":
            worst_plain = max(worst_plain, float(np.abs(p_m - p_t).max()))
        elif (c.H, c.W) != (c.hs, c.ws):
            assert np.abs(p_t - ref.probs).max() > 1e-6, c.name
            apart.append(float(np.abs(p_m - p_t).max()))
    assert worst_plain < 5e-7 and max(apart) > 2e-6 and np.median(apart) > 2e-6


def test_coords_follow_aten_definition():
    i0, step, lam = sr.coords(300, 1200)
    scale = np.float32(299) / np.float32(1199)
    for d in (0, 1, 599, 1198, 1199):
        src = np.float32(scale * np.float32(d))
        assert i0[d] == int(src) and lam[d] == np.float32(src - np.float32(int(src))) and step[d] == (int(src) < 299)
    assert lam.dtype == np.float32 and (lam >= 0).all() and (lam < 1).all() and (i0 + step <= 299).all()
    i0, step, lam = sr.coords(7, 1)
    assert i0.tolist() == [0] and lam.tolist() == [0.0]
    i0, step, lam = sr.coords(1, 5)
    assert i0.tolist() == [0] * 5 and step.tolist() == [0] * 5 and lam.tolist() == [0.0] * 5
    # identity: weights exactly 0, the reference returns the input itself
    x = sr.logits(1, 3, 12, 10, 3)
    up, M = sr.upsample64(x, 12, 10)
    assert (up == x.astype(np.float64)).all()
    assert (torch.from_numpy(sr.upsample_f32_model(x, 12, 10)) == torch.from_numpy(x)).all()
