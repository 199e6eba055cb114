"""tests/layer_ref.py pinned on the CPU: the restatements against torch's own convolutions, the case table against the sources' selector
rules, and the conditions that make the exact fixtures of tests/test_gpu_layer_kernels.py independent of every summation order."""
import os
import re

import pytest
import torch

from tests import layer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional
_r16 = lambda t: t.to(torch.bfloat16).double()


@pytest.mark.parametrize("ksize,stride,with_res,with_x2", [(1, 1, True, False), (1, 2, False, False), (3, 1, False, False), (3, 2, False, False),
                                                          (1, 1, False, 1), (1, 1, True, 2)])
def test_layer_is_torchs_convolution_on_the_packed_weight_layout(ksize, stride, with_res, with_x2):
    g = torch.Generator().manual_seed(11 * ksize + stride + 2 * with_x2)
    B, H, W, Cin, Cout, pad = 2, 6, 8, 16, 24, ksize // 2
    x = _r16(torch.randn(B, H, W, Cin, generator=g))
    C2 = 8 if with_x2 else 0
    w = _r16(torch.randn(Cout, ksize * ksize * Cin + C2, generator=g) / 4)
    bias = torch.randn(Cout, generator=g).double()
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    res = _r16(torch.randn(B, Ho, Wo, Cout, generator=g)) if with_res else None
    x2 = _r16(torch.randn(B, Ho * with_x2, Wo * with_x2, C2, generator=g)) if with_x2 else None
    K1 = ksize * ksize * Cin
    want = F.conv2d(x.permute(0, 3, 1, 2), w[:, :K1].view(Cout, ksize, ksize, Cin).permute(0, 3, 1, 2), bias, stride=stride, padding=pad)
    if with_x2:
        want = want + F.conv2d(x2.permute(0, 3, 1, 2), w[:, K1:, None, None], None, stride=with_x2)
    want = want.permute(0, 2, 3, 1)
    if with_res:
        want = want + res
    got, mag = R.layer(x, w, bias, ksize, stride, pad, True, res, x2, with_x2 or 1)
    assert got.dtype == torch.float64 and got.shape == (B, Ho, Wo, Cout) == mag.shape
    assert float((got - torch.relu(want)).abs().max()) < 1e-12 and float(got.max()) > 1.0 and bool((got == 0).any())
    raw, _ = R.layer(x, w, bias, ksize, stride, pad, False, res, x2, with_x2 or 1)
    assert float((raw - want).abs().max()) < 1e-12 and bool((mag >= raw.abs()).all())
    assert R.layer(x, w, bias, ksize, stride, pad, True, res, x2, with_x2 or 1, dtype=torch.float32)[0].dtype == torch.float32


@pytest.mark.parametrize("stride2", [2, 1])
def test_stage_first_is_torchs_two_layers(stride2):
    g = torch.Generator().manual_seed(40 + stride2)
    B, H, Cm, C2 = 2, 8, 8, 16
    t1 = _r16(torch.randn(B, H, H, Cm, generator=g))
    x2 = _r16(torch.randn(B, H // 2 * stride2, H // 2 * stride2, C2, generator=g))
    w2, wc = _r16(torch.randn(Cm, 9 * Cm, generator=g) / 8), _r16(torch.randn(4 * Cm, Cm + C2, generator=g) / 4)
    b2, bc = torch.randn(Cm, generator=g).double(), torch.randn(4 * Cm, generator=g).double()
    t2 = R.bf16_rne(torch.relu(F.conv2d(t1.permute(0, 3, 1, 2), w2.view(Cm, 3, 3, Cm).permute(0, 3, 1, 2), b2, stride=2, padding=1)))
    want = torch.relu(F.conv2d(t2, wc[:, :Cm, None, None], bc) + F.conv2d(x2.permute(0, 3, 1, 2), wc[:, Cm:, None, None], None, stride=stride2))
    got, parts = R.stage_first(t1, x2, w2, b2, wc, bc, stride2, parts=True)
    assert got.shape == (B, H // 2, H // 2, 4 * Cm) and float((got - want.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    assert torch.equal(parts["t2"], t2.permute(0, 2, 3, 1))
    # the two layer launches the kernel replaces, restated one by one, are the same function
    a, _ = R.layer(t1, w2, b2, 3, 2, 1)
    b, _ = R.layer(R.bf16_rne(a), wc, bc, x2=x2, stride2=stride2)
    assert torch.equal(b, got)


def test_kernel_ids_are_the_headers_enum():
    text = open(os.path.join(ROOT, "ivos-w_amd", "csrc", "conv.h")).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"enum ConvKernel \{(.*?)\};", text, re.S).group(1))
    ids = [s.strip() for s in body.split(",") if s.strip()]
    assert ids[-1] == "CK_COUNT" and tuple(ids[:-1]) == R.CONV_KERNELS


def test_case_table_reaches_what_it_names_and_everything_it_must():
    """Every row's `reaches` is what the sources' own rules give for that shape, frame count and tunables; the rows together reach every bf16 id
    of the selector but the stem, both NPT forms of the wide kernel, both RES forms of the 8-phase kernel and stage_first."""
    ids = [R.case_id(c, B) for c, B in R.case_params()]
    assert len(ids) == len(set(ids))
    for c, B in R.case_params():
        assert set(c.tune) <= set(R.DEFAULTS), c
        assert R.expected(c, B) == c.reaches, (R.case_id(c, B), R.expected(c, B))
        assert 1 <= B <= 5
        if c.path != "sf":
            l = R.LAYERS[c.layer]
            assert l.Cin % 64 == 0 and (l.Cout == 64 or l.Cout % 128 == 0) and (l.x2 is None or (l.ksize == 1 and (R.out_hw(l) - 1) * l.x2[2] < l.x2[0]))
            if c.path in ("wide", "g8"):           # conv1x1_wide_ok / conv1x1_g8_ok on the shape
                Ho = R.out_hw(l)
                assert l.ksize == 1 and l.Cout % 256 == 0 and R.k_total(l) >= 384 and Ho * Ho * (l.Cout // 256) >= 256
                assert c.path == "wide" or (l.stride == 1 and R.k_total(l) % 128 == 0)
    assert {c.reaches for c in R.CASES} == R.MUST_REACH
    assert set(R.BF16_SELECTOR_IDS) == set(R.CONV_KERNELS) - {"CK_STEM", "CK_PATCH_X3"}
    # tiles: every tiled path meets a launch that is no multiple of its tile and one of more than one tile
    for name in ("red5", "p512", "exp5", "cat5"):
        Ho = R.out_hw(R.LAYERS[name])
        ms = {B * Ho * Ho for c in R.CASES if c.layer == name for B in c.frames}
        assert any(m % 256 for m in ms) and any(m > 256 for m in ms), name


def _exact_names():
    return sorted({(c.layer, B) for c, B in R.case_params()})


@pytest.mark.parametrize("name,B", _exact_names())
def test_exact_fixture_is_exact_in_any_summation_order(name, B):
    fx = R.exact_fixture(name, B)
    sf = name in R.SF_ARMS
    tensors = list(fx) if sf else [v for v in fx.values() if v is not None]
    for t in tensors:                       # operands: small integers, so bf16 holds them
        assert torch.equal(t, t.round()) and torch.equal(t, t.to(torch.bfloat16).float())
    weights = [fx[2], fx[4]] if sf else [fx["w"]]
    for w in weights:                       # K coverage: every K index (the x2 part included) meets a nonzero weight, every row has 8 or 9
        nz = w != 0
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert bool(nz.any(dim=0).all()) and set(nz.sum(dim=1).tolist()) <= {8, 9}
    acts = [fx[0], fx[1]] if sf else [fx[k] for k in ("x", "x2", "res") if fx[k] is not None]
    for a in acts:                          # activations differ by channel parity, and no frame repeats another
        assert int(a[..., 0::2].min()) == -3 and int(a[..., 0::2].max()) == 3 and int(a[..., 1::2].min()) == -1 and int(a[..., 1::2].max()) == 2
        assert len({hash(a[b].numpy().tobytes()) for b in range(B)}) == B
    if sf:
        pre, parts = R.sf_ref(name, fx, parts=True)
        a2 = parts["a2"]                    # t2 before its rounding: integers of magnitude <= 256, so the rounding is the identity
        assert torch.equal(a2, a2.round()) and float(a2.abs().max()) <= 256 and torch.equal(parts["t2"], torch.relu(a2))
        assert 0.25 < float((a2 > 0).double().mean()) < 0.75
        mags = parts["mag"]
        r32 = R.sf_ref(name, fx, torch.float32)
        l = None
    else:
        l = R.LAYERS[name]
        assert int((fx["w"].view(l.Cout, 9, l.Cin) != 0).sum(dim=2).min()) == 1 if l.ksize == 3 else True       # every tap of every row
        pre, mag = R.layer_ref(name, fx)
        mags = (mag,)
        r32 = R.layer_ref(name, fx, torch.float32)[0]
        raw = R.layer(fx["x"], fx["w"], fx["bias"], l.ksize, l.stride, l.pad, False, fx["res"], fx["x2"], l.x2[2] if l.x2 else 1)[0]
        assert 0.25 < float((raw > 0).double().mean()) < 0.75 and bool((raw < 0).any())                       # both ReLU branches
    # sum of |terms| below 2^24: every fp32 partial sum is an exactly represented integer in any order
    for m in mags:
        assert float(m.max()) < 2 ** 24
    # |ref64| <= 256: bf16 holds the integer exactly, so a single wrong term cannot round away
    assert torch.equal(pre, pre.round()) and float(pre.abs().max()) <= 256
    assert torch.equal(R.bf16_rne(pre), pre)
    assert r32.dtype == torch.float32 and torch.equal(r32.double(), pre)
    assert 0.25 < float((pre > 0).double().mean()) < 0.75 and len(pre.unique()) >= 12
    want = R.exact_want(name, B)
    assert want.shape == pre.shape and torch.equal(want.double(), pre)


@pytest.mark.parametrize("name", sorted({c.layer for c in R.CASES}))
def test_dense_fixture_and_its_yardsticks(name):
    fx = R.dense_fixture(name)
    sf = name in R.SF_ARMS
    tensors = [fx[0], fx[1], fx[2], fx[4]] if sf else [fx[k] for k in ("x", "w", "res", "x2") if fx[k] is not None]
    for t in tensors:
        assert torch.equal(t, t.to(torch.bfloat16).float())                      # operands are bf16 values
    acts = [fx[0], fx[1]] if sf else [fx[k] for k in ("x", "res", "x2") if fx[k] is not None]
    for a in acts:
        assert float(a.min()) >= 0 and 0.3 < float((a > 0).float().mean()) < 0.7    # post-ReLU tensors
        assert a.shape[0] >= R.max_frames(name)
    if sf:
        assert fx[0].shape[0] * 32 * 32 * 128 >= R.DENSE_T1
        p64, p32 = (R.sf_ref(name, fx, dt, parts=True)[1] for dt in (torch.float64, torch.float32))
        flips = int((p64["t2"] != p32["t2"].double()).sum())
        r64, r32, d32 = R.dense_refs(name)
        print(f"\n{name}: {fx[0].shape[0]} frames, t2 flips {flips}, d32 {d32:.3e}")
        assert flips >= 8 and d32 > 2e-4                                           # what flips cost, against ~1e-5 of fp32 noise
        for B in (1, 3):                                                          # ref32 itself, rounded, sits inside both bounds
            ratio, mean, _, m32 = R.sf_figures(R.bf16_rne(r32[:B]), name, B)
            assert ratio <= 1.0 and mean == m32 and 1e-3 < m32 < 2e-2
        return
    r64, mag, r32 = R.dense_refs(name)
    assert bool((mag >= r64.abs()).all()) and 0.2 < float((r64 > 0).double().mean()) < 0.9
    for B in sorted({B for c in R.CASES if c.layer == name for B in c.frames}):
        ratio, mean, m32 = R.layer_figures(R.bf16_rne(r32[:B]), name, B)
        assert ratio <= 1.0 and mean == m32 and m32 > 1e-4, (ratio, mean, m32)
        # the bound is tight enough to see one wrong element: bf16_rne(ref64) is inside, the same with one element moved by 5 % is not
        y = R.bf16_rne(r64[:B]).float()
        assert R.layer_figures(y, name, B)[0] <= 1.0
        y[0, 0, 0, 0] += 0.05 * max(1.0, float(y[0, 0, 0, 0]))
        assert R.layer_figures(y, name, B)[0] > 1.0
