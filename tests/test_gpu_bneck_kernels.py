"""The fused bottleneck kernels of csrc/bottleneck.hip and csrc/bottleneck_wide.hip, each ALONE through the probe entries
(include/ivosw_probe.h, libivosw_probe.so), every output element against the float64 restatement of tests/bneck_ref.py
(pinned on the CPU by tests/test_bneck_ref.py):

  exact   small-integer operands whose sums no fp32 order can change: y == bf16_rne(ref64) bit for bit
  dense   the probe tools' random recipe: every element within 2^-8 |ref64| + 4 * d32, the mean within 1.5 * m32, with d32 / m32
          measured from the float32 and float64 restatements alone (bneck_ref.dense_figures)
  both    y sits between two guard frames, everything pre-filled with a NaN pattern: finite inside, untouched outside
  refuse  shapes and arms the probes must refuse return an error and leave y as it was

The probe library is a second copy of the sources with its own tunables: arms are chosen through ITS ivosw_tune_set and put back.
The wide probe also reorders the K-major weights into fragment order on the device (launch_fragpack), so its cases cover that too.
Frame counts hit the grid arithmetic: one frame, an odd count, and for res5 the two-frames-per-workgroup packing.
"""
import contextlib

import pytest
import torch

from ivos_w_amd import _lib as L
from tests import bneck_ref as R

pytestmark = pytest.mark.gpu

# name -> the arms that reach a kernel of their own at that shape: (label, {tunable: value}); defaults as the sources read them
DEFAULTS = {"HALO64S": 1, "HALO_WLDS": 1, "HALO128S": 0, "HALF16_MAX": 96, "FUSE_WIDE5": 0}
ARMS = {
    "id64": [("bneck64<256,false>", {})],
    "ds64": [("bneck64<64,true>", {})],
    "res2": [("halo64s<false,false,0>", {"HALO64S": 1}), ("halo<64>", {"HALO64S": 0})],
    "res3": [("halo<128,true>", {}), ("halo<128>", {"HALO_WLDS": 0}), ("halo128s", {"HALO128S": 1})],
    "res4": [("half16", {}), ("wide<256,16,1>", {"HALF16_MAX": 0})],
}
RES5_ARMS = {0: ("wide<512,8,2>", {"FUSE_WIDE5": 1}), 1: ("wide<512,8,1>", {"FUSE_WIDE5": 2})}      # by B % 2


def _cases():
    out = []
    for name, B, H in R.shape_cases():
        arms = [RES5_ARMS[B % 2]] if name == "res5" else ARMS[name]
        out += [pytest.param(name, B, H, tune, id=f"{name}-B{B}-H{H}-{label}") for label, tune in arms]
    return out


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
            assert lib.ivosw_tune_set(k.encode(), DEFAULTS[k]) == 0


def _launch(dev, lib, fx, B, H, Cin, Cm, wide):
    """One probe launch, ts NULL.  Returns (status, the int16 view of [guard frame | y | guard frame])."""
    x, wa, ba, wb, bb, wc, bc, wd, bd = fx
    h = lambda t: None if t is None else t.to(torch.bfloat16).to(dev).contiguous()
    f = lambda t: None if t is None else t.float().to(dev).contiguous()
    p = lambda t: None if t is None else L.dptr(t)
    dx, dwa, dwb, dwc, dwd = h(x), h(wa), h(wb), h(wc), h(wd)
    dba, dbb, dbc, dbd = f(ba), f(bb), f(bc), f(bd)
    buf = torch.full((B + 2, H, H, 4 * Cm), R.NAN_BITS, dtype=torch.int16, device=dev)
    y = buf[1:B + 1]
    st = L.stream_ptr(dev)
    if wide:
        assert wd is None
        frag = torch.full((2 * (2 * Cm * Cin + 9 * Cm * Cm) + 256,), 0xA5, dtype=torch.uint8, device=dev)   # three weight copies + 256 B
        frag[-256:] = 0                                                                                     # ... of zeros
        rc = lib.ivosw_bneck_wide_probe(p(dx), p(y), p(dwa), p(dba), p(dwb), p(dbb), p(dwc), p(dbc), p(frag), B, H, H, Cin, Cm, None, st)
    else:
        zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
        rc = lib.ivosw_bneck_probe(p(dx), p(y), p(dwa), p(dba), p(dwb), p(dbb), p(dwc), p(dbc), p(dwd), p(dbd), p(zeros), B, H, H, Cin, Cm, None, st)
    torch.cuda.synchronize(dev)
    return rc, buf.cpu()


def _run(dev, name, B, H, tune, fx):
    """The case's launch with its checks on status, guards and finiteness; returns y [B,H,H,4*Cmid] as float32 on the CPU."""
    entry, Cin, Cm = R.SHAPES[name][:3]
    with _tuned(tune) as lib:
        rc, buf = _launch(dev, lib, fx, B, H, Cin, Cm, entry == "w")
        assert rc == 0, lib.ivosw_last_error().decode()
    assert bool((buf[0] == R.NAN_BITS).all()) and bool((buf[-1] == R.NAN_BITS).all()), "guard frame written"
    y = buf[1:B + 1].contiguous().view(torch.bfloat16).float()
    assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} elements not written or not finite"
    return y


@pytest.mark.parametrize("name,B,H,tune", _cases())
def test_exact_fixture_is_bit_equal_to_fp64(dev, name, B, H, tune):
    """Integer operands (bneck_ref.exact_fixture: every fp32 partial sum exact in any order, t1 / t2 unchanged by their rounding):
    every element of y equals bf16_rne(ref64), zero tolerance."""
    y = _run(dev, name, B, H, tune, R.exact_fixture(name, B, H))
    want = R.exact_want(name, B, H)
    bad = y != want
    if bool(bad.any()):
        idx = bad.nonzero()
        b, r, c, ch = idx[0].tolist()
        pytest.fail(f"{int(bad.sum())} of {bad.numel()} elements differ; frames {sorted(set(idx[:, 0].tolist()))}, rows {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, "
                    f"cols {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, {len(set(idx[:, 3].tolist()))} channels; first at (b {b}, y {r}, x {c}, ch {ch}): "
                    f"got {float(y[b, r, c, ch])}, want {float(want[b, r, c, ch])}")
    assert torch.equal(y.to(torch.bfloat16).view(torch.int16), want.to(torch.bfloat16).view(torch.int16))       # -0 would differ here


@pytest.mark.parametrize("name,B,H,tune", _cases())
def test_dense_fixture_is_within_one_fp32_reordering_of_fp64(dev, name, B, H, tune):
    """Random operands: |y - ref64| <= 2^-8 |ref64| + 4 * d32 for every element and mean |y - ref64| <= 1.5 * m32, where
    d32 = max |ref32 - ref64| (over the shape's dense batch of >= 2^19 t1 values, of which the kernel runs the first B frames) and
    m32 = mean |bf16_rne(ref32) - ref64| (over those B frames) come from the two CPU restatements alone.

    Measured on the MI355X (LAB_NOTES.md has every case): worst element 0.23 ... 0.54 of its bound, mean 0.997 ... 1.011 m32."""
    y = _run(dev, name, B, H, tune, R.dense_case(name, B, H))
    ratio, mean, d32, m32 = R.dense_figures(y, name, B, H)
    print(f"\n{name} B={B} H={H} {tune}: d32 {d32:.3e}  m32 {m32:.3e}  worst |y-ref64| / bound {ratio:.3f}  mean |y-ref64| {mean:.3e} = {mean / m32:.3f} m32")
    assert ratio <= 1.0, f"an element is {ratio:.2f} x its bound (d32 {d32:.3e})"
    assert mean <= 1.5 * m32, f"mean error {mean:.3e} against m32 {m32:.3e}"


def _refused(dev, name, B, H, tune, Cin=None, Cm=None):
    entry, cin, cm = R.SHAPES[name][:3]
    Cin, Cm = Cin or cin, Cm or cm
    g = torch.Generator().manual_seed(7)
    fx = (torch.randn(B, H, H, Cin, generator=g), torch.randn(Cm, Cin, generator=g), torch.zeros(Cm), torch.randn(Cm, 9 * Cm, generator=g),
          torch.zeros(Cm), torch.randn(4 * Cm, Cm, generator=g), torch.zeros(4 * Cm), None, None)
    with _tuned(tune) as lib:
        rc, buf = _launch(dev, lib, fx, B, H, Cin, Cm, entry == "w")
        err = lib.ivosw_last_error().decode()
    assert rc != 0 and "not covered" in err, (rc, err)
    assert bool((buf == R.NAN_BITS).all()), "a refused call wrote y"


def test_res5_is_refused_unless_asked_for(dev):
    """FUSE_WIDE5 = 0, the default: the res5 shape is not the wide kernel's (the tower runs its three layer kernels)."""
    _refused(dev, "res5", 2, 8, {})
    _refused(dev, "res5", 2, 8, {"FUSE_WIDE5": 0})


def test_res5_two_frame_form_refuses_an_odd_batch(dev):
    _refused(dev, "res5", 3, 8, {"FUSE_WIDE5": 1})


def test_bneck_probe_refuses_a_frame_that_is_no_multiple_of_its_tile(dev):
    _refused(dev, "id64", 1, 24, {})


def test_wide_probe_refuses_cin_other_than_four_cmid(dev):
    _refused(dev, "res4", 1, 16, {}, Cin=512, Cm=256)
