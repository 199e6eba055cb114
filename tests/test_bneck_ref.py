"""tests/bneck_ref.py pinned on the CPU: the restatement against torch's own convolutions, its bf16 rounding at ties, and the
conditions that make the exact fixtures of tests/test_gpu_bneck_kernels.py independent of every summation order."""
import pytest
import torch

from tests import bneck_ref as R


def test_bf16_rne_float64_rounds_once_and_ties_to_even():
    v = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, -257.0, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([256.0, 256.0, 258.0, 260.0, 260.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -256.0, 0.0], dtype=torch.float64)
    assert torch.equal(R.bf16_rne(v), want)
    # through float32 the value 2^-40 above the tie would be rounded twice and land on the even neighbour below
    assert float(v[6].float().to(torch.bfloat16)) == 1.0
    f = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    assert torch.equal(R.bf16_rne(f.double()).float(), f.to(torch.bfloat16).float())
    assert torch.equal(R.bf16_rne(f), f.to(torch.bfloat16).float())


@pytest.mark.parametrize("ds", [False, True])
def test_block_is_torchs_bottleneck_on_the_probes_weight_layout(ds):
    """The matrix form here (3 x 3 taps gathered along K = (ky*3 + kx)*Cmid + c) against conv2d on the view the probe tools take of
    the same wb, in float64 where the summation order cannot flip a bf16 rounding of t1 / t2 at these sizes."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(5 + ds)
    B, H, W, Cin, Cm = 2, 5, 7, 16 if ds else 32, 8
    r16 = lambda t: t.to(torch.bfloat16).double()
    x = r16(torch.randn(B, H, W, Cin, generator=g))
    wa, wb, wc = r16(torch.randn(Cm, Cin, generator=g) / 4), r16(torch.randn(Cm, 9 * Cm, generator=g) / 8), r16(torch.randn(4 * Cm, Cm, generator=g) / 3)
    ba, bb, bc = (torch.randn(n, generator=g).double() for n in (Cm, Cm, 4 * Cm))
    wd, bd = (r16(torch.randn(4 * Cm, Cin, generator=g) / 4), torch.randn(4 * Cm, generator=g).double()) if ds else (None, None)
    xf = x.permute(0, 3, 1, 2)
    t1 = R.bf16_rne(torch.relu(F.conv2d(xf, wa[:, :, None, None], ba)))
    t2 = R.bf16_rne(torch.relu(F.conv2d(t1, wb.view(Cm, 3, 3, Cm).permute(0, 3, 1, 2), bb, padding=1)))
    idt = F.conv2d(xf, wd[:, :, None, None], bd) if ds else xf
    want = torch.relu(F.conv2d(t2, wc[:, :, None, None], bc) + idt).permute(0, 2, 3, 1)
    got = R.ref64(x, wa, ba, wb, bb, wc, bc, wd, bd)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-12
    assert float(got.max()) > 1.0


@pytest.mark.parametrize("name,B,H", R.shape_cases())
def test_exact_fixture_is_exact_in_any_summation_order(name, B, H):
    fx = R.exact_fixture(name, B, H)
    x, wa, ba, wb, bb, wc, bc, wd, bd = fx
    # operands: small integers, so bf16 holds them; x differs by channel parity
    for t in fx:
        if t is not None:
            assert torch.equal(t, t.round()) and torch.equal(t, t.to(torch.bfloat16).float())
    assert int(x[..., 0::2].min()) == -3 and int(x[..., 0::2].max()) == 3 and int(x[..., 1::2].min()) == -1 and int(x[..., 1::2].max()) == 2
    # K coverage: every K index of every layer meets a nonzero weight, every output row has one
    for w in (wa, wb, wc) + ((wd,) if wd is not None else ()):
        nz = w != 0
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert bool(nz.any(dim=0).all()) and bool(nz.any(dim=1).all())
    assert int((wb.view(-1, 9, wa.shape[0]) != 0).sum(dim=2).min()) == 1           # every tap of every row
    pre, parts = R.block(*fx, dtype=torch.float64, parts=True)
    # t1 / t2 before rounding: integers of magnitude <= 256, so their bf16 rounding is the identity
    for a in (parts["a1"], parts["a2"]):
        assert torch.equal(a, a.round()) and float(a.abs().max()) <= 256
        assert torch.equal(R.bf16_rne(torch.relu(a)), torch.relu(a))
    # every layer: sum of |terms| below 2^24, so every fp32 partial sum is an exactly represented integer in any order
    for m in parts["mag"]:
        assert float(m.max()) < 2 ** 24
    assert torch.equal(pre, pre.round())
    r32 = R.ref32(*fx)
    assert r32.dtype == torch.float32 and torch.equal(r32.double(), pre)
    # the fixture is not trivial: a good share of every layer is alive and spread over many values (the outputs stay small
    # enough that their own bf16 rounding is mostly the identity: that rounding is the dense fixture's business)
    want = R.exact_want(name, B, H)
    assert float((parts["a1"] > 0).double().mean()) > 0.25 and float((parts["a2"] > 0).double().mean()) > 0.25
    assert float((pre > 0).double().mean()) > 0.25
    assert len(pre.unique()) > 48 and float(pre.max()) <= 2 ** 24
    # no frame, and no tile of a frame, repeats another
    assert len({hash(x[b].numpy().tobytes()) for b in range(B)}) == B
    if H >= 32:
        assert not torch.equal(want[:, :16], want[:, 16:32]) and not torch.equal(want[:, :, :16], want[:, :, 16:32])


@pytest.mark.parametrize("name,H", sorted({(n, H) for n, _, H in R.shape_cases()}))
def test_dense_batch_measures_rounding_flips(name, H):
    """d32 is meant to be the cost of one legitimate fp32 reordering - a flipped bf16 rounding of t1 and what follows from it - so
    ref32 and ref64 must disagree on t1 and t2 values of every dense batch (>= 2^19 t1 values); d32 is then far above fp32 noise,
    and the mean is the output's own bf16 rounding."""
    fx = R.dense_fixture(name, H)
    assert fx[0].shape[0] * H * H * R.SHAPES[name][2] >= R.DENSE_T1 and fx[0].shape[0] >= max(B for n, B, h in R.shape_cases() if (n, h) == (name, H))
    for t in fx[1::2][:3] + (fx[0],) + ((fx[7],) if fx[7] is not None else ()):
        assert torch.equal(t, t.to(torch.bfloat16).float())                      # operands are bf16 values
    p64, p32 = (R.block(*fx, dtype=dt, parts=True)[1] for dt in (torch.float64, torch.float32))
    flips = [int((p64[k] != p32[k].double()).sum()) for k in ("t1", "t2")]
    r64, r32, d32 = R.dense_refs(name, H)
    print(f"\n{name} H={H}: {fx[0].shape[0]} frames, t1 / t2 flips {flips}, d32 {d32:.3e}")
    assert flips[0] >= 2 and flips[1] >= 2
    assert d32 > 1e-3                                                            # what flips cost, against ~1e-5 of fp32 noise
    # ref32 itself, rounded, sits inside both bounds for every frame count of the shape
    for B in sorted(B for n, B, h in R.shape_cases() if (n, h) == (name, H)):
        ratio, mean, _, m32 = R.dense_figures(R.bf16_rne(r32[:B]), name, B, H)
        assert ratio <= 1.0 and mean == m32 and 1e-3 < m32 < 1e-2
