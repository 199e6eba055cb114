"""The single-layer kernels of the default bf16 tower - conv_igemm_dma_kernel, conv_igemm_ws_kernel, conv3x3_patch_kernel (csrc/conv.hip),
conv1x1_wide_kernel (csrc/bottleneck_wide.hip), gemm_8phase_kernel (csrc/gemm_8phase.h) - and stage_first_kernel (csrc/stage_first.hip),
each ALONE through ivosw_conv_probe / ivosw_stage_first_probe (include/ivosw_probe.h, libivosw_probe.so), every output element against the
float64 restatement of tests/layer_ref.py (pinned on the CPU by tests/test_layer_ref.py), on one to five frames of the tower's own layer
geometry (the case table is layer_ref.CASES):

  reach   the probe reports the instantiation that ran: it is the one the table's row names, and the rows together reach every one
  exact   small-integer operands whose sums no fp32 order can change: y == bf16_rne(ref64) bit for bit
  dense   a layer: |y - ref64| <= 2^-8 max(|ref64|, |y|) + (K + 2) 2^-23 mag per element (the output's bf16 rounding + the worst case of an
          fp32 sum of K + 2 terms in any order) and mean |y - ref64| <= 1.5 m32; stage_first (t2 is rounded on the way): the bottleneck
          kernels' rule, 2^-8 |ref64| + 4 d32 and 1.5 m32.  Every yardstick comes from the CPU restatements alone.
  rev     the descending tile order gives the same bits
  guards  y, x, x2 and res each sit between guard frames of a NaN pattern: y's stay untouched, the inside is finite - a tail tile that let a
          row past M or a neighbouring frame's pixel into an output would show as a NaN
  refuse  what a kernel does not take is refused ("not covered") and nothing is written

The probe library is a second copy of the sources with its own tunables: arms are chosen through ITS ivosw_tune_set and put back."""
import contextlib
import ctypes

import pytest
import torch

from ivos_w_amd import _lib as L
from tests import layer_ref as R

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(c, B, id=R.case_id(c, B)) for c, B in R.case_params()]
KERNEL = {"sel": 0, "wide": 1, "g8": 2}
REACHED = {}            # case id -> what the probe reported (test_the_table_reached_every_instantiation reads it)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _tuned(tune):
    lib = L.probe_lib()
    try:
        for k, v in tune.items():
            assert lib.ivosw_tune_set(k.encode(), int(v)) == 0
        yield lib
    finally:
        for k in tune:
            assert lib.ivosw_tune_set(k.encode(), R.DEFAULTS[k]) == 0


def _guarded(t, dev):
    """bf16 copy of t [B,...] on the device between two guard frames of the NaN pattern; returns (whole buffer, the view of the B frames)."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), R.NAN_BITS, dtype=torch.int16, device=dev)
    buf[1:-1] = t.to(torch.bfloat16).view(torch.int16).to(dev)
    return buf, buf[1:-1]


def _ybuf(B, Ho, Cout, dev):
    return torch.full((B + 2, Ho, Ho, Cout), R.NAN_BITS, dtype=torch.int16, device=dev)


def _frag(nbytes, dev):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)


def _launch_layer(dev, lib, l, fx, B, kernel, rev=0, geom=None):
    """One ivosw_conv_probe call.  Returns (status, reported id, [guard | y | guard] as int16 on the CPU, frag on the CPU)."""
    p = lambda t: None if t is None else L.dptr(t)
    keep = [_guarded(fx[k], dev) if fx[k] is not None else (None, None) for k in ("x", "res", "x2")]
    (_, dx), (_, dres), (_, dx2) = keep
    dw, dbias = fx["w"].to(torch.bfloat16).to(dev).contiguous(), fx["bias"].float().to(dev).contiguous()
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
    frag = _frag(dw.numel() * 2, dev)
    buf = _ybuf(B, R.out_hw(l), l.Cout, dev)
    ran = ctypes.c_int(-1)
    H2, C2, s2 = l.x2 if l.x2 else (0, 0, 0)
    ksize, stride, pad = geom or (l.ksize, l.stride, l.pad)
    rc = lib.ivosw_conv_probe(p(dx), p(dw), p(dbias), p(dres), p(dx2), p(buf[1:-1]), p(zeros), p(frag), B, l.H, l.H, l.Cin, l.Cout, ksize, stride, pad, 1, rev,
                              H2, H2, C2, s2, kernel, ctypes.byref(ran), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, ran.value, buf.cpu(), frag.cpu()


def _launch_sf(dev, lib, name, fx, B, rev=0, Ho=32):
    p = L.dptr
    t1, x2, w2, b2, wc, bc = fx
    (_, dt1), (_, dx2) = keep = [_guarded(t1, dev), _guarded(x2, dev)]
    dw2, dwc = (w.to(torch.bfloat16).to(dev).contiguous() for w in (w2, wc))
    db2, dbc = b2.float().to(dev).contiguous(), bc.float().to(dev).contiguous()
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
    frag = _frag((dw2.numel() + dwc.numel()) * 2, dev)
    buf = _ybuf(B, 32, 512, dev)
    H2, s2 = R.SF_ARMS[name]
    rc = lib.ivosw_stage_first_probe(p(dt1), p(dx2), p(dw2), p(db2), p(dwc), p(dbc), p(frag), p(zeros), p(buf[1:-1]), B, Ho, Ho, H2, H2, s2, rev, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    del keep
    return rc, buf.cpu(), frag.cpu()


def _run(dev, c, B, fx, rev=0):
    """The case's launch with its checks on status, reported instantiation, guards and finiteness; returns y as float32 on the CPU."""
    with _tuned(c.tune) as lib:
        if c.path == "sf":
            rc, buf, _ = _launch_sf(dev, lib, c.layer, fx, B, rev)
            got = "SF"
        else:
            rc, ran, buf, _ = _launch_layer(dev, lib, R.LAYERS[c.layer], fx, B, KERNEL[c.path], rev)
            got = R.reported(c, ran) if rc == 0 else None
        assert rc == 0, lib.ivosw_last_error().decode()
    REACHED[R.case_id(c, B)] = got
    assert got == c.reaches, f"the launch ran {got}, the table names {c.reaches}"
    assert bool((buf[0] == R.NAN_BITS).all()) and bool((buf[-1] == R.NAN_BITS).all()), "guard frame written"
    y = buf[1:-1].contiguous().view(torch.bfloat16).float()
    assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} elements not written or not finite"
    return y


def _bits(y):
    return y.to(torch.bfloat16).view(torch.int16)


@pytest.mark.parametrize("c,B", PARAMS)
def test_exact_fixture_is_bit_equal_to_fp64(dev, c, B):
    """Integer operands (layer_ref.exact_fixture: every fp32 partial sum exact in any order, |ref64| <= 256): every element of y equals
    bf16_rne(ref64), zero tolerance."""
    y = _run(dev, c, B, R.exact_fixture(c.layer, B))
    want = R.exact_want(c.layer, B)
    bad = y != want
    if bool(bad.any()):
        idx = bad.nonzero()
        b, r, col, ch = idx[0].tolist()
        pytest.fail(f"{int(bad.sum())} of {bad.numel()} elements differ; frames {sorted(set(idx[:, 0].tolist()))}, rows {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, "
                    f"cols {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, {len(set(idx[:, 3].tolist()))} channels; first at (b {b}, y {r}, x {col}, ch {ch}): "
                    f"got {float(y[b, r, col, ch])}, want {float(want[b, r, col, ch])}")
    assert torch.equal(_bits(y), _bits(want))       # -0 would differ here


@pytest.mark.parametrize("c,B", PARAMS)
def test_dense_fixture_is_within_its_derived_bound_of_fp64(dev, c, B):
    """Random operands, activations >= 0.  A layer: |y - ref64| <= 2^-8 max(|ref64|, |y|) + (K + 2) 2^-23 mag for every element;
    stage_first: |y - ref64| <= 2^-8 |ref64| + 4 d32 (d32 = max |ref32 - ref64| over 2^20 t2 values); both: mean |y - ref64| <= 1.5 m32.
    And the launch in descending tile order gives the same bits.

    Measured on the MI355X (LAB_NOTES.md has every case): a layer's worst element 0.43 ... 0.99 of its bound, stage_first's 0.44 ... 0.53,
    the mean 1.000 m32 in all 124 cases."""
    fx = R.first_frames(R.dense_fixture(c.layer), B)
    y = _run(dev, c, B, fx)
    if c.path == "sf":
        ratio, mean, d32, m32 = R.sf_figures(y, c.layer, B)
    else:
        ratio, mean, m32 = R.layer_figures(y, c.layer, B)
    print(f"\nFIG {R.case_id(c, B)}: m32 {m32:.3e}  worst |y-ref64| / bound {ratio:.3f}  mean |y-ref64| {mean:.3e} = {mean / m32:.3f} m32")
    assert ratio <= 1.0, f"an element is {ratio:.2f} x its bound"
    assert mean <= 1.5 * m32, f"mean error {mean:.3e} against m32 {m32:.3e}"
    assert torch.equal(_bits(_run(dev, c, B, fx, rev=1)), _bits(y)), "rev = 1 changed bits"


def test_the_table_reached_every_instantiation(dev):
    """Every bf16 ConvKernel id but the stem, both NPT forms of the wide kernel, both RES forms of the 8-phase kernel, stage_first: each
    reported by a launch of its own (one frame of every row, exact operands - the full cases above fill in the rest when they ran first)."""
    for c in R.CASES:
        B = c.frames[0]
        if R.case_id(c, B) not in REACHED:
            _run(dev, c, B, R.exact_fixture(c.layer, B))
    assert set(REACHED.values()) == set(R.MUST_REACH), sorted(set(R.MUST_REACH) - set(REACHED.values()))


def test_stage_first_equals_its_two_layer_launches_bit_for_bit(dev):
    """stage_first.hip promises the layer kernels' K order: on the dense fixture its output equals the 3x3 stride-2 layer launch (selector)
    followed by the [conv3 | downsample] wide launch on that launch's t2, bit for bit - kernel alone, not through taps of the tower."""
    for name, (H2, s2) in R.SF_ARMS.items():
        for B in (1, 3):
            fx = R.first_frames(R.dense_fixture(name), B)
            t1, x2, w2, b2, wc, bc = fx
            lib = L.probe_lib()
            rc, buf, _ = _launch_sf(dev, lib, name, fx, B)
            assert rc == 0, lib.ivosw_last_error().decode()
            l3 = R.LAYERS["s2_128"]
            rc, _, t2buf, _ = _launch_layer(dev, lib, l3, {"x": t1, "w": w2, "bias": b2, "res": None, "x2": None}, B, 0)
            assert rc == 0, lib.ivosw_last_error().decode()
            t2 = t2buf[1:-1].contiguous().view(torch.bfloat16).float()
            lc = R.Layer("cat3_" + name, 32, 128, 512, 1, 1, 0, False, (H2, 256, s2))
            rc, ran, ybuf, _ = _launch_layer(dev, lib, lc, {"x": t2, "w": wc, "bias": bc, "res": None, "x2": x2}, B, 1)
            assert rc == 0 and ran == 8, lib.ivosw_last_error().decode()
            assert torch.equal(buf, ybuf), f"{name} B={B}: {int((buf != ybuf).sum())} elements differ"


def _refused_layer(dev, name, kernel, geom=None):
    l = R.LAYERS[name]
    lib = L.probe_lib()
    rc, ran, buf, frag = _launch_layer(dev, lib, l, R.exact_fixture(name, 1), 1, kernel, geom=geom)
    err = lib.ivosw_last_error().decode()
    assert rc != 0 and "not covered" in err, (rc, err)
    assert ran == -1 and bool((buf == R.NAN_BITS).all()) and bool((frag == 0xA5).all()), "a refused call wrote y or frag"


def test_wide_kernel_refuses_res5s_reduction(dev):
    """2048 -> 512 at 8 x 8 is half a workgroup per frame: conv1x1_wide_ok's workgroup rule turns it down."""
    _refused_layer(dev, "red5", 1)


def test_wide_kernel_refuses_a_3x3(dev):
    # the probe's y and the operands keep the 1x1 geometry's sizes: ksize 3 with pad 1 at stride 1 asks for the same frames
    _refused_layer(dev, "red4", 1, geom=(3, 1, 1))


def test_8phase_kernel_refuses_stride_2(dev):
    # (a refused call touches no tensor: y keeps the stride-1 size)
    _refused_layer(dev, "red4", 2, geom=(1, 2, 0))


def test_stage_first_probe_refuses_another_frame_size(dev):
    lib = L.probe_lib()
    rc, buf, frag = _launch_sf(dev, lib, "sf_s2", R.exact_fixture("sf_s2", 1), 1, Ho=16)
    err = lib.ivosw_last_error().decode()
    assert rc != 0 and "not covered" in err, (rc, err)
    assert bool((buf == R.NAN_BITS).all()) and bool((frag == 0xA5).all()), "a refused call wrote y or frag"
