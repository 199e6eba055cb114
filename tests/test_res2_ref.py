"""tests/res2_ref.py pinned on the CPU: the restatements against torch's own convolutions and pooling, the chain kernel's bias split, the
case tables, and the conditions that make the exact fixtures of tests/test_gpu_res2_stem_kernels.py independent of every summation order."""
import pytest
import torch

from tests import bneck_ref as BR
from tests import res2_ref as R

F = torch.nn.functional
_r16 = lambda t: t.to(torch.bfloat16).double()


def _small_res2(g, H=6, W=7):
    x = _r16(torch.relu(torch.randn(2, H, W, 64, generator=g)))
    ws = tuple(_r16(torch.randn(r, k, generator=g) / k ** 0.5) for r, k in R.W_SHAPES)
    bs = tuple(0.3 * torch.randn(s[0], generator=g) for s in R.W_SHAPES)
    return x, ws, bs


@pytest.mark.parametrize("form", [0, 1])
def test_res2_is_torchs_three_bottlenecks_and_the_forwarded_conv1(form):
    x, ws, bs = _small_res2(torch.Generator().manual_seed(21 + form))
    e = R.kernel_biases(bs, form)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    c1 = lambda t, w, b: F.conv2d(t, w.double()[:, :, None, None], b)
    h = nchw(x)
    for k in range(3):
        t1 = R.bf16_rne(torch.relu(c1(h, ws[k], e[k])))
        t2 = R.bf16_rne(torch.relu(F.conv2d(t1, ws[4 + k].double().view(64, 3, 3, 64).permute(0, 3, 1, 2), e[4 + k], padding=1)))
        idt = F.conv2d(h, ws[10].double()[:, :, None, None]) if k == 0 else h
        pre = torch.relu(c1(t2, ws[7 + k], e[7 + k]) + idt)
        h = R.bf16_rne(pre)
    t1out = torch.relu(c1(h, ws[3], e[3]))
    y, t, parts = R.res2(x, ws, bs, form=form, parts=True)
    assert y.dtype == torch.float64 and y.shape == (2, 6, 7, 256) and t.shape == (2, 6, 7, 128)
    assert float((y - pre.permute(0, 2, 3, 1)).abs().max()) < 1e-12 and float((t - t1out.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    assert torch.equal(parts["blocks"][2]["y"], R.bf16_rne(y)) and float(y.max()) > 1.0 and bool((t == 0).any())
    y32, t32 = R.res2(x, ws, bs, form=form, dtype=torch.float32)
    assert y32.dtype == torch.float32 and float((y32.double() - y).abs().max()) < 0.1


def test_chain_bias_is_hi_plus_lo_and_block0_conv3_takes_the_fp32_sum():
    g = torch.Generator().manual_seed(23)
    bs = tuple(0.1 * torch.randn(s[0], generator=g) for s in R.W_SHAPES)
    e0, e1 = R.kernel_biases(bs, 0), R.kernel_biases(bs, 1)
    assert len(e0) == len(e1) == 10 and all(t.dtype == torch.float64 for t in e0 + e1)
    cat = bs[7] + bs[10]                                            # fp32, as concat_k_kernel and res2_chain_pack_kernel add them
    assert torch.equal(e0[7], cat.double()) and not torch.equal(e0[7], bs[7].double() + bs[10].double())
    for i, b in enumerate(bs[:7] + (cat, bs[8], bs[9])):
        hi, lo = R.split_bias(b)
        assert torch.equal(hi, b.to(torch.bfloat16).float()) and torch.equal(lo, (b - hi).to(torch.bfloat16).float())
        assert torch.equal(e1[i], hi.double() + lo.double()) and torch.equal(e1[i].float().double(), e1[i])      # exact in fp32
        assert torch.equal(e0[i], b.double())
        d = (e1[i] - b.double()).abs()
        assert bool((d > 0).any()) and bool((d <= 2.0 ** -16 * b.double().abs()).all())        # not b, but within two bf16 roundings of it
        assert bool((lo != 0).float().mean() > 0.9)


def test_stem_is_torchs_convolution_and_max_pool_and_the_bank_layout():
    g = torch.Generator().manual_seed(25)
    roi = _r16(torch.randn(2, 24, 20, 4, generator=g))
    w, bias = _r16(torch.randn(64, 196, generator=g) / 14), torch.randn(64, generator=g)
    conv = F.conv2d(roi.permute(0, 3, 1, 2), w.view(64, 7, 7, 4).permute(0, 3, 1, 2), bias.double(), stride=2, padding=3)
    want = F.max_pool2d(R.bf16_rne(torch.relu(conv)), 3, 2, 1).permute(0, 2, 3, 1)
    pre, mag, a = R.stem(roi, w, bias, parts=True)
    assert pre.shape == (2, 6, 5, 64) == mag.shape and a.shape == (2, 12, 10, 64)
    assert float((a - conv.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    assert torch.equal(R.bf16_rne(pre), want)                       # rounding before or after the maximum: the same bits
    assert bool((mag >= pre).all()) and bool((pre >= 0).all()) and bool((pre == 0).any())
    bank = R.pack_stem(w)
    assert bank.shape == (64, 8, 8, 4) and not bank[:, 7].any() and not bank[:, :, 7].any()
    assert float(bank[5, 3, 2, 1]) == float(w[5, (3 * 7 + 2) * 4 + 1])


def test_case_tables_cover_kinds_phases_tile_walks_and_every_reported_value():
    ids = [R.case_id(c) for c in R.EXACT_CASES] + [R.case_id(c, True) + "-dense" for c in R.DENSE_CASES]
    assert len(ids) == len(set(ids))
    assert {R.reported(c) for c in R.EXACT_CASES} == R.MUST_REACH == {R.reported(c) for c in R.DENSE_CASES}
    for kind, (form, tune, _) in R.KINDS.items():
        assert set(tune) <= set(R.DEFAULTS) and form in (0, 1)
        ex = [c for c in R.EXACT_CASES if c.kind == kind]
        assert {(c.phase, c.y_s2) for c in ex if not c.frac} == {(p, s) for p in range(R.PHASES) for s in (0, 1)}      # every phase, both y forms
        assert {c.y_s2 for c in ex if c.frac} == {0, 1} and {c.B for c in ex} == {1, 2, R.BIG}
        assert {c.rev for c in ex} == {0, 1}
        de = [c for c in R.DENSE_CASES if c.kind == kind]
        assert {c.B for c in de} == {1, 2} and {c.y_s2 for c in de} == {0, 1} and any(c.phase == 1 for c in de)
    assert R.KINDS["chain5"][1] == {"R2C_GRID": 5} and R.KINDS["chain1"][1] == {"R2C_PERSIST": 0}
    # the tile walk: 32 tiles per frame; 5 workgroups own 6 or 7 of one frame's; one frame above CUs / 32 leaves workgroups with 2 tiles and with 1
    assert sorted({(32 - L + 4) // 5 for L in range(5)}) == [6, 7]
    n = R.frames(R.BIG) * 32
    assert R.frames(R.BIG) == R.BIG_CPU and 256 < n < 512 and R.frames(3) == 3 and R.frames(R.BIG, 304) == 10
    assert max(R.STEM_EXACT_FRAMES) * 64 > 512 and min(R.STEM_EXACT_FRAMES) == 1        # the stem's persistent grid is 512 workgroups
    assert R.DENSE_FRAMES * 64 * 64 * 64 >= R.DENSE_T1 and R.DENSE_FRAMES >= max(c.B for c in R.DENSE_CASES)


def test_exact_weights_phases_put_a_nonzero_on_every_k_index():
    seen = [torch.zeros(k, dtype=torch.bool) for _, k in R.W_SHAPES]
    for phase in range(R.PHASES):
        ws = R.exact_fixture(1, phase).ws
        for i, (w, (rows, k)) in enumerate(zip(ws, R.W_SHAPES)):
            nz = w != 0
            assert w.shape == (rows, k) and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
            assert set(nz.sum(dim=1).tolist()) == {3 if k == 576 else 2}
            if k == 576:                                            # one tap per filter row, another column of it in every phase
                assert bool((nz.view(rows, 3, 192).sum(dim=2) == 1).all())
            seen[i] |= nz.any(dim=0)
    assert all(bool(s.all()) for s in seen), [R.W_NAMES[i] for i, s in enumerate(seen) if not bool(s.all())]
    a, b = R.exact_fixture(1, 0).ws, R.exact_fixture(1, 1).ws
    assert not any(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("phase,frac", [(0, False), (1, False), (2, False), (1, True)])
def test_exact_fixture_is_exact_in_any_summation_order(phase, frac):
    fx = R.exact_fixture(1, phase, frac)
    unit = 2.0 ** -10 if frac else 1.0                               # everything is a multiple of `unit` ...
    cap = 2.0 ** 14 if frac else 2.0 ** 24                           # ... and every sum of |terms| below 2^24 units
    for t in (fx.x,) + fx.ws:
        assert torch.equal(t, t.round()) and torch.equal(t, t.to(torch.bfloat16).float())
    assert int(fx.x.min()) == -2 and int(fx.x.max()) == 2
    for b in fx.bs:
        n = b - (2.0 ** -10 if frac else 0.0)
        assert torch.equal(n, n.round()) and float(n.abs().max()) <= 4
        if frac:                                                    # no bf16 value, exact as hi + lo, the low half alive
            hi, lo = R.split_bias(b)
            assert torch.equal(hi + lo, b) and bool(((lo != 0) | (n == 0)).all()) and not torch.equal(b, b.to(torch.bfloat16).float())
    whole = lambda t: torch.equal(t / unit, (t / unit).round())
    for form in (0, 1):
        y, t, parts = R.res2(*fx, form=form, parts=True)
        for p in parts["blocks"]:
            for a in (p["a1"], p["a2"]):
                assert whole(a) and float(a.abs().max()) <= 256
            for r in (p["t1"], p["t2"], p["y"]):                    # every rounded tensor: |v| <= 256
                assert whole(r) and float(r.abs().max()) <= 256 and float((r > 0).double().mean()) > 0.25
            if not frac:                                            # integers <= 256: the roundings are the identity, an error of 1 shows
                assert torch.equal(p["t1"], torch.relu(p["a1"])) and torch.equal(p["t2"], torch.relu(p["a2"]))
            for m in p["mag"]:
                assert float(m.max()) < cap
        assert whole(parts["a4"]) and float(parts["mag4"].max()) < cap and float(t.max()) <= 256 and float(y.max()) <= 256
        if not frac:
            assert torch.equal(R.bf16_rne(y), y) and torch.equal(R.bf16_rne(t), t)
        y32, t32 = R.res2(*fx, form=form, dtype=torch.float32)
        assert torch.equal(y32.double(), y) and torch.equal(t32.double(), t)            # one fp32 order gives ref64 itself
        for v in (y, t):
            assert 0.25 < float((v > 0).double().mean()) < 0.9 and len(v.unique()) >= 24
        wy, wt = R.exact_want(1, phase, frac, form)
        assert torch.equal(wy.double(), R.bf16_rne(y)) and torch.equal(wt.double(), R.bf16_rne(t))
        print(f"\nphase {phase} frac {frac} form {form}: max y0 .. y2 {[float(p['y'].max()) for p in parts['blocks']]}, t1out {float(t.max())}")
    w0, w1 = R.exact_want(1, phase, frac, 0), R.exact_want(1, phase, frac, 1)
    assert torch.equal(w0[0], w1[0]) and torch.equal(w0[1], w1[1])                      # exact biases: both forms add the same values
    # no tile of the frame repeats another, and the even-pixel form is no copy of a corner
    assert not torch.equal(w0[0][:, :8], w0[0][:, 8:16]) and not torch.equal(w0[0][:, :, :16], w0[0][:, :, 16:32])
    if frac:
        # the chain kernel's low bias half is under the zero-tolerance test: with hi alone both outputs change
        hi_only = tuple(R.split_bias(b)[0] for b in fx.bs)
        y, t = R.res2(fx.x, fx.ws, hi_only, form=1)
        ny, nt = int((R.bf16_rne(y).float() != w1[0]).sum()), int((R.bf16_rne(t).float() != w1[1]).sum())
        print(f"hi-only biases change {ny} elements of y and {nt} of t1out")
        assert ny > 1000 and nt > 1000


def test_exact_frames_differ_and_larger_counts_are_cheap():
    fx = R.exact_fixture(R.BIG_CPU, 2)
    assert len({hash(fx.x[b].numpy().tobytes()) for b in range(R.BIG_CPU)}) == R.BIG_CPU
    wy, wt = R.exact_want(R.BIG_CPU, 2, False, 1)
    assert wy.shape == (R.BIG_CPU, 64, 64, 256) and wt.shape == (R.BIG_CPU, 64, 64, 128) and float(wy.max()) <= 256


def test_stem_exact_fixture_is_exact_in_any_summation_order():
    roi, w, bias = R.stem_exact_fixture(3)
    for t in (roi, w, bias):
        assert torch.equal(t, t.round()) and torch.equal(t, t.to(torch.bfloat16).float())
    assert int(roi.min()) == -3 and int(roi.max()) == 3 and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert bool((w != 0).any(dim=0).all()) and set((w != 0).sum(dim=1).tolist()) == {14}                # all 196 K indices
    assert bool(((w != 0).view(64, 7, 28).sum(dim=2) == 2).all())
    pre, mag, a = R.stem(roi, w, bias, parts=True)
    assert torch.equal(a, a.round()) and float(a.abs().max()) <= 256 and float(mag.max()) < 2 ** 24
    assert torch.equal(R.bf16_rne(pre), pre) and len(pre.unique()) >= 12 and bool((a < 0).any())
    r32 = R.stem(roi, w, bias, dtype=torch.float32)[0]
    assert torch.equal(r32.double(), pre) and torch.equal(R.stem_exact_want(3).double(), pre)
    assert len({hash(roi[b].numpy().tobytes()) for b in range(3)}) == 3
    assert not torch.equal(pre[:, :8], pre[:, 8:16]) and not torch.equal(pre[:, :, :8], pre[:, :, 8:16])


def _relu_bias_border(fx, form):
    """The wrong kernel the border case is there for: block 0's t1 outside the frame is relu(bias) instead of the 3x3's zero padding."""
    x, ws, bs = fx
    e = R.kernel_biases(bs, form)
    xd = x.double()
    t1 = R.bf16_rne(torch.relu(xd @ ws[0].double().t() + e[0]))
    B, H, W, C = t1.shape
    p = R.bf16_rne(torch.relu(e[0])).expand(B, H + 2, W + 2, C).clone()
    p[:, 1:-1, 1:-1] = t1
    k2 = torch.cat([p[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=-1)
    t2 = R.bf16_rne(torch.relu(k2 @ ws[4].double().t() + e[4]))
    h = R.bf16_rne(torch.relu(t2 @ ws[7].double().t() + e[7] + xd @ ws[10].double().t()))
    for k in (1, 2):
        h = R.bf16_rne(BR.block(h, ws[k], e[k], ws[4 + k], e[4 + k], ws[7 + k], e[7 + k]))
    return h.float(), R.bf16_rne(torch.relu(h @ ws[3].double().t() + e[3])).float()


@pytest.mark.parametrize("pos", [0, 1])
def test_dense_fixture_and_its_yardsticks(pos):
    fx = R.dense_fixture(pos)
    for t in (fx.x,) + fx.ws:
        assert torch.equal(t, t.to(torch.bfloat16).float())                              # operands are bf16 values
    assert float(fx.x.min()) >= 0 and 0.3 < float((fx.x > 0).float().mean()) < 0.7        # the pooled stem output
    assert fx.x.shape[0] == R.DENSE_FRAMES and fx.x.shape[0] * 64 * 64 * 64 >= R.DENSE_T1
    assert all(not torch.equal(b, b.to(torch.bfloat16).float()) for b in fx.bs)          # biases are NOT bf16 values
    if pos:
        assert all(float(b.min()) >= 0.5 for b in fx.bs[:7])
    for form in (0, 1):
        p64, p32 = (R.res2(*fx, form=form, dtype=dt, parts=True)[2] for dt in (torch.float64, torch.float32))
        flips = [int((p64["blocks"][0][k] != p32["blocks"][0][k].double()).sum()) for k in ("t1", "t2")]
        r64, r32, d32 = R.dense_refs(pos, form)
        print(f"\npos {pos} form {form}: block 0 t1 / t2 flips {flips}, d32 y {d32[0]:.3e} t1out {d32[1]:.3e}")
        assert flips[0] >= 2 and flips[1] >= 2 and min(d32) > 1e-3                       # what flips cost, against ~1e-5 of fp32 noise
        kind = "stage" if form == 0 else "chain"
        for c in R.DENSE_CASES:
            if c.kind != kind or c.phase != pos:
                continue
            s = 2 if c.y_s2 else 1
            # ref32 itself, rounded, sits inside both bounds ...
            figs = R.dense_figures(R.bf16_rne(r32[0][:c.B, ::s, ::s]), R.bf16_rne(r32[1][:c.B]), c)
            for ratio, mean, _, m32 in figs:
                assert ratio <= 1.0 and mean == m32 and 1e-3 < m32 < 0.25, (ratio, mean, m32)     # (y2 is ~ 30 on average, up to ~ 600)
            # ... and so does bf16_rne(ref64), but not with one element moved by 5 % and two margins of the reordering term
            y, t = R.bf16_rne(r64[0][:c.B, ::s, ::s]).float(), R.bf16_rne(r64[1][:c.B]).float()
            assert all(f[0] <= 1.0 for f in R.dense_figures(y, t, c))
            y[0, 0, 0, 0] += 0.05 * max(1.0, float(y[0, 0, 0, 0])) + 8 * d32[0]
            t[0, 1, 1, 1] += 0.05 * max(1.0, float(t[0, 1, 1, 1])) + 8 * d32[1]
            assert all(f[0] > 1.0 for f in R.dense_figures(y, t, c))
    # the two forms' references differ (hi + lo is not b) but by far less than either bound
    dy = float((R.dense_refs(pos, 0)[0][0] - R.dense_refs(pos, 1)[0][0]).abs().max())
    assert 0 < dy
    if pos:
        # the border case: a halo pixel that took relu(bias) leaves the per-element bound in y and in t1out
        c = next(c for c in R.DENSE_CASES if c.kind == "chain" and c.phase == 1)
        one = R.Res2Fx(fx.x[:c.B].contiguous(), fx.ws, fx.bs)
        y, t = _relu_bias_border(one, 1)
        figs = R.dense_figures(y, t, c)
        print(f"relu(bias) in block 0's halo: y at {figs[0][0]:.1f} x its bound, t1out at {figs[1][0]:.1f} x")
        assert figs[0][0] > 2.0 and figs[1][0] > 2.0


def test_stem_dense_fixture_and_its_yardsticks():
    roi, w, bias = R.stem_dense_fixture()
    for t in (roi, w):
        assert torch.equal(t, t.to(torch.bfloat16).float())
    assert float(roi[..., 3].min()) >= 0 and float(roi[..., 3].max()) <= 1 and float(roi[..., :3].min()) < -1
    assert roi.shape[0] == max(R.STEM_DENSE_FRAMES)
    r64, mag, r32 = R.stem_dense_refs()
    assert bool((mag >= r64.abs()).all()) and float((r64 > 0).double().mean()) > 0.5
    for B in R.STEM_DENSE_FRAMES:
        ratio, mean, m32 = R.stem_figures(R.bf16_rne(r32[:B]), B)
        assert ratio <= 1.0 and mean == m32 and m32 > 1e-4, (ratio, mean, m32)
        y = R.bf16_rne(r64[:B]).float()
        assert R.stem_figures(y, B)[0] <= 1.0
        y[0, 0, 0, 0] += 0.05 * max(1.0, float(y[0, 0, 0, 0]))
        assert R.stem_figures(y, B)[0] > 1.0
