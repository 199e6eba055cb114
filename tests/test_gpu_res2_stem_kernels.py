"""The three kernels of the default bf16 tower's front that no per-element test reached - res2_chain_kernel (csrc/res2_chain.hip: the
default res2 path), res2_stage_kernel (csrc/res2_stage.hip: its RES2_CHAIN=0 fallback) and stem_pool_kernel (csrc/stem.hip) - each ALONE
through ivosw_res2_probe / ivosw_stem_probe (include/ivosw_probe.h, libivosw_probe.so) on the caller's weights, every output element of y,
t1out and the pooled map against the float64 restatement of tests/res2_ref.py (pinned on the CPU by tests/test_res2_ref.py):

  exact   small-integer operands whose sums no fp32 order can change (three phases of weight placement that together put a nonzero on every K
          index of every layer, and a variant with biases n + 2^-10 that only the chain kernel's (hi, lo) bias split holds exactly): y and
          t1out == bf16_rne(ref64) bit for bit, both res2 forms, y_s2 0 and 1, and the stem
  dense   res2 (t1, t2 and y of three blocks are rounded on the way): the bottleneck kernels' rule, |out - ref64| <= 2^-8 |ref64| + 4 d32 per
          element and mean <= 1.5 m32, for y and for t1out; stem: the layer rule, 2^-8 max(|ref64|, |out|) + (K + 2) 2^-23 mag with mag the
          largest sum of |terms| in the pool window, and mean <= 1.5 m32.  Every yardstick comes from the CPU restatements alone.
  rev     the descending tile order gives the same bits
  forms   the chain kernel one tile per workgroup (R2C_PERSIST=0), persistent on 5 workgroups (R2C_GRID=5: 6 or 7 tiles of a frame each) and
          persistent by default give identical bits; the stage kernel sums in another order and is held to fp64 like them, not to them
  walk    1 frame (one tile per workgroup, no next tile), 2 frames on 5 workgroups, and one frame more than CUs / 32 (9 on the MI355X: under the
          default grid some workgroups own two tiles, some one); the stem on 1, 3 and 9 frames (576 tiles on 512 workgroups: the register
          prefetch of a second tile).  The large counts run the exact fixture only.
  guards  y, t1out, x, the pooled map and the ROI tiles each sit between guard frames of a NaN pattern: the outputs' stay untouched, the inside
          is finite - a halo row taken from a neighbouring frame, a tile past B or a pending t1out tile stored at the wrong boundary would show
  border  one dense fixture has every conv1 and conv2 bias >= 0.5: a halo pixel outside the frame that took relu(bias) instead of the 3x3's
          zero padding puts y at 6.9 x and t1out at 4.9 x the per-element bound (tests/test_res2_ref.py computes that wrong kernel on the CPU),
          so the per-element bound catches it; in the exact fixtures about half of those biases are positive and any such pixel breaks bit equality
  reach   every *ran value the probe can report - stage, chain one tile per workgroup, chain persistent, each with y_s2 0 and 1 - is reached
  refuse  a NULL operand (also among the weight pointers), B <= 0 or another form: an error, nothing launched, y, t1out and frag untouched

The probe library is a second copy of the sources with its own tunables: arms are chosen through ITS ivosw_tune_set and put back."""
import contextlib
import ctypes

import pytest
import torch

from ivos_w_amd import _lib as L
from tests import res2_ref as R

pytestmark = pytest.mark.gpu

R_NW = L.RES2_PROBE_NW
REACHED = {}            # case id -> the *ran value the probe reported (test_every_reported_value_was_reached reads it)


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


def _frames(dev, B):
    return R.frames(B, torch.cuda.get_device_properties(dev).multi_processor_count)


def _guarded(t, dev):
    """bf16 copy of t [B,...] on the device between two guard frames of the NaN pattern; returns (whole buffer, the view of the B frames)."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), R.NAN_BITS, dtype=torch.int16, device=dev)
    buf[1:-1] = t.to(torch.bfloat16).view(torch.int16).to(dev)
    return buf, buf[1:-1]


def _nanbuf(shape, dev):
    return torch.full(shape, R.NAN_BITS, dtype=torch.int16, device=dev)


def _bits(y):
    return y.to(torch.bfloat16).view(torch.int16)


def _launch_res2(dev, lib, fx, B, form, y_s2, rev=0, null=None, Bcall=None):
    """One ivosw_res2_probe call on the first B frames' worth of buffers.  null: "x" or ("w" | "b", i) passes a NULL there; Bcall: the frame
    count handed to the probe when it is not B.  Returns (status, ran, [guard | y | guard], [guard | t1out | guard], frag), on the CPU."""
    xbuf, dx = _guarded(fx.x[:B], dev)
    dws = [w.to(torch.bfloat16).to(dev).contiguous() for w in fx.ws]
    dbs = [b.float().to(dev).contiguous() for b in fx.bs]
    wp, bp = [t.data_ptr() for t in dws], [t.data_ptr() for t in dbs]
    if isinstance(null, tuple):
        (wp if null[0] == "w" else bp)[null[1]] = None
    warr, barr = (ctypes.c_void_p * R_NW)(*wp), (ctypes.c_void_p * R_NW)(*bp)
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
    frag = torch.full((L.RES2_PROBE_FRAG_BYTES,), 0xA5, dtype=torch.uint8, device=dev)
    hy = 32 if y_s2 else 64
    ybuf, tbuf = _nanbuf((B + 2, hy, hy, 256), dev), _nanbuf((B + 2, 64, 64, 128), dev)
    ran = ctypes.c_int(-1)
    rc = lib.ivosw_res2_probe(None if null == "x" else L.dptr(dx), warr, barr, L.dptr(frag), L.dptr(zeros), L.dptr(ybuf[1:-1]), L.dptr(tbuf[1:-1]),
                              B if Bcall is None else Bcall, y_s2, rev, form, ctypes.byref(ran), L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    del xbuf
    return rc, ran.value, ybuf.cpu(), tbuf.cpu(), frag.cpu()


def _inside(buf, what):
    assert bool((buf[0] == R.NAN_BITS).all()) and bool((buf[-1] == R.NAN_BITS).all()), f"guard frame of {what} written"
    v = buf[1:-1].contiguous().view(torch.bfloat16).float()
    assert bool(torch.isfinite(v).all()), f"{int((~torch.isfinite(v)).sum())} elements of {what} not written or not finite"
    return v


def _run_res2(dev, c, fx, B, rev=None, dense=False):
    """The case's launch with its checks on status, reported instantiation, guards and finiteness; returns (y, t1out) as float32 on the CPU."""
    form, tune, _ = R.KINDS[c.kind]
    with _tuned(tune) as lib:
        rc, ran, ybuf, tbuf, _ = _launch_res2(dev, lib, fx, B, form, c.y_s2, c.rev if rev is None else rev)
        assert rc == 0, lib.ivosw_last_error().decode()
    REACHED[R.case_id(c, dense) + ("-dense" if dense else "")] = ran
    assert ran == R.reported(c), f"the launch reported {ran}, the table names {R.reported(c)}"
    return _inside(ybuf, "y"), _inside(tbuf, "t1out")


def _assert_bit_equal(got, want, what):
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()
        b, r, col, ch = idx[0].tolist()
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; frames {sorted(set(idx[:, 0].tolist()))}, rows {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, "
                    f"cols {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, {len(set(idx[:, 3].tolist()))} channels; first at (b {b}, y {r}, x {col}, ch {ch}): "
                    f"got {float(got[b, r, col, ch])}, want {float(want[b, r, col, ch])}")
    assert torch.equal(_bits(got), _bits(want)), f"{what}: a -0"       # -0 would differ here


# ---------------------------------------------------------------- res2
@pytest.mark.parametrize("c", [pytest.param(c, id=R.case_id(c)) for c in R.EXACT_CASES])
def test_res2_exact_fixture_is_bit_equal_to_fp64(dev, c):
    """Integer operands (res2_ref.exact_fixture: every fp32 partial sum exact in any order, every rounded tensor <= 256; the frac variant in
    units of 2^-10): every element of y and of t1out equals bf16_rne(ref64), zero tolerance."""
    B = _frames(dev, c.B)
    y, t = _run_res2(dev, c, R.exact_fixture(B, c.phase, c.frac), B)
    wy, wt = R.exact_want(B, c.phase, c.frac, R.KINDS[c.kind][0])
    _assert_bit_equal(t, wt, "t1out")
    _assert_bit_equal(y, wy[:, ::2, ::2] if c.y_s2 else wy, "y")


@pytest.mark.parametrize("c", [pytest.param(c, id=R.case_id(c, True)) for c in R.DENSE_CASES])
def test_res2_dense_fixture_is_within_the_bottleneck_bound_of_fp64(dev, c):
    """Random operands, x >= 0, biases that are no bf16 values; "pos": every conv1 / conv2 bias >= 0.5 (the border case).  For y and for t1out:
    |out - ref64| <= 2^-8 |ref64| + 4 d32 for every element (d32 = max |ref32 - ref64| over the 2^19 block-0 t1 values of the dense batch) and
    mean |out - ref64| <= 1.5 m32.  And the launch in descending tile order gives the same bits.

    Measured on the MI355X (LAB_NOTES.md has every case): the worst element of y 0.20 ... 0.33 of its bound, of t1out 0.24 ... 0.28; the mean
    0.98 ... 1.02 m32 in all 12 cases; the three chain forms give the same figures (the same bits)."""
    fx = R.dense_fixture(c.phase)
    y, t = _run_res2(dev, c, fx, c.B, dense=True)
    figs = R.dense_figures(y, t, c)
    for name, (ratio, mean, d32, m32) in zip(("y", "t1out"), figs):
        print(f"\nFIG res2 {R.case_id(c, True)} {name}: d32 {d32:.3e}  m32 {m32:.3e}  worst |out-ref64| / bound {ratio:.3f}  mean |out-ref64| {mean:.3e} = {mean / m32:.3f} m32")
    for name, (ratio, mean, d32, m32) in zip(("y", "t1out"), figs):
        assert ratio <= 1.0, f"an element of {name} is {ratio:.2f} x its bound"
        assert mean <= 1.5 * m32, f"{name}: mean error {mean:.3e} against m32 {m32:.3e}"
    yr, tr = _run_res2(dev, c, fx, c.B, rev=1, dense=True)
    assert torch.equal(_bits(yr), _bits(y)) and torch.equal(_bits(tr), _bits(t)), "rev = 1 changed bits"


@pytest.mark.parametrize("y_s2", [0, 1])
def test_res2_chain_forms_give_identical_bits(dev, y_s2):
    """One tile per workgroup, persistent on 5 workgroups and persistent on one workgroup per CU are the same arithmetic per tile: the ring that
    runs across tile boundaries, the prefetched p halo and the deferred t1out stores change no bit - on the dense fixture (2 frames, both tile
    orders) and on the exact fixture at the large frame count."""
    def bits(kind, fx, B, rev):
        y, t = _run_res2(dev, R.Case(kind, B, y_s2, 0, False, rev), fx, B)
        return _bits(y), _bits(t)
    big = _frames(dev, R.BIG)
    for fx, B, rev in ((R.dense_fixture(0), 2, 0), (R.dense_fixture(0), 2, 1), (R.exact_fixture(big, 0, False), big, 0)):
        ref = bits(R.CHAIN_KINDS[0], fx, B, rev)
        for kind in R.CHAIN_KINDS[1:]:
            got = bits(kind, fx, B, rev)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"{kind} differs from {R.CHAIN_KINDS[0]} (B {B}, rev {rev})"


def test_every_reported_value_was_reached(dev):
    """Every *ran value of ivosw_res2_probe - res2_stage_kernel, res2_chain_kernel one tile per workgroup and persistent, each with y_s2 0 and 1 -
    was reported by a launch (one frame of the exact fixture fills in what the cases above did not run first)."""
    for c in R.EXACT_CASES:
        if R.reported(c) not in REACHED.values():
            B = _frames(dev, c.B)
            _run_res2(dev, c, R.exact_fixture(B, c.phase, c.frac), B)
    assert set(REACHED.values()) == set(R.MUST_REACH), sorted(set(R.MUST_REACH) - set(REACHED.values()))


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("what", ["x", "w3", "b10", "B0", "Bneg"])
def test_res2_probe_refuses_before_it_launches(dev, form, what):
    null = {"x": "x", "w3": ("w", 3), "b10": ("b", 10)}.get(what)
    Bcall = {"B0": 0, "Bneg": -2}.get(what)
    lib = L.probe_lib()
    rc, ran, ybuf, tbuf, frag = _launch_res2(dev, lib, R.exact_fixture(1, 0, False), 1, form, 0, null=null, Bcall=Bcall)
    err = lib.ivosw_last_error().decode()
    assert rc != 0 and ("null" in err or "B must" in err), (rc, err)
    assert ran == -1 and bool((ybuf == R.NAN_BITS).all()) and bool((tbuf == R.NAN_BITS).all()) and bool((frag == 0xA5).all()), "a refused call wrote y, t1out or frag"


def test_res2_probe_refuses_another_form(dev):
    lib = L.probe_lib()
    rc, ran, ybuf, tbuf, frag = _launch_res2(dev, lib, R.exact_fixture(1, 0, False), 1, 2, 0)
    assert rc != 0 and "form" in lib.ivosw_last_error().decode()
    assert ran == -1 and bool((ybuf == R.NAN_BITS).all()) and bool((tbuf == R.NAN_BITS).all()) and bool((frag == 0xA5).all())


# ---------------------------------------------------------------- stem
def _launch_stem(dev, lib, fx, B, rev=0, null=False, Bcall=None):
    roi, w, bias = fx
    rbuf, droi = _guarded(roi[:B], dev)
    bank = R.pack_stem(w).to(torch.bfloat16).to(dev).contiguous()
    dbias = bias.float().to(dev).contiguous()
    obuf = _nanbuf((B + 2, 64, 64, 64), dev)
    rc = lib.ivosw_stem_probe(None if null else L.dptr(droi), L.dptr(bank), L.dptr(dbias), L.dptr(obuf[1:-1]), B if Bcall is None else Bcall, rev, L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    del rbuf
    return rc, obuf.cpu()


def _run_stem(dev, fx, B, rev=0):
    lib = L.probe_lib()
    rc, obuf = _launch_stem(dev, lib, fx, B, rev)
    assert rc == 0, lib.ivosw_last_error().decode()
    return _inside(obuf, "the pooled map")


@pytest.mark.parametrize("B", R.STEM_EXACT_FRAMES)
def test_stem_exact_fixture_is_bit_equal_to_fp64(dev, B):
    """Integer ROI in [-3,3], filters in {-1,0,+1} that meet all 196 K indices, integer biases, conv values <= 256: the pooled map equals
    bf16_rne(ref64) bit for bit, in both tile orders.  9 frames are 576 tiles on 512 workgroups: 64 of them fetch a second patch."""
    want = R.stem_exact_want(B)
    for rev in (0, 1):
        _assert_bit_equal(_run_stem(dev, R.stem_exact_fixture(B), B, rev), want, f"pooled map (rev {rev})")


@pytest.mark.parametrize("B", R.STEM_DENSE_FRAMES)
def test_stem_dense_fixture_is_within_the_layer_bound_of_fp64(dev, B):
    """Random ROI tiles (three signed colour channels, mask probability in [0,1]), randn / sqrt(K) filters: |out - ref64| <=
    2^-8 max(|ref64|, |out|) + (196 + 2) 2^-23 mag per element, mag the largest sum of |terms| in the pool window, and mean <= 1.5 m32; the
    descending tile order gives the same bits.

    Measured on the MI355X (LAB_NOTES.md): the worst element 0.972 of its bound at 1 and at 3 frames, the mean 1.000 m32."""
    fx = R.stem_dense_fixture()
    out = _run_stem(dev, fx, B)
    ratio, mean, m32 = R.stem_figures(out, B)
    print(f"\nFIG stem B{B}: m32 {m32:.3e}  worst |out-ref64| / bound {ratio:.3f}  mean |out-ref64| {mean:.3e} = {mean / m32:.3f} m32")
    assert ratio <= 1.0, f"an element is {ratio:.2f} x its bound"
    assert mean <= 1.5 * m32, f"mean error {mean:.3e} against m32 {m32:.3e}"
    assert torch.equal(_bits(_run_stem(dev, fx, B, rev=1)), _bits(out)), "rev = 1 changed bits"


@pytest.mark.parametrize("what", ["roi", "B0", "Bneg"])
def test_stem_probe_refuses_before_it_launches(dev, what):
    lib = L.probe_lib()
    rc, obuf = _launch_stem(dev, lib, R.stem_exact_fixture(1), 1, null=what == "roi", Bcall={"B0": 0, "Bneg": -1}.get(what))
    err = lib.ivosw_last_error().decode()
    assert rc != 0 and ("null" in err or "B must" in err), (rc, err)
    assert bool((obuf == R.NAN_BITS).all()), "a refused call wrote the pooled map"
