"""res4's chained identity blocks (bneck_wide_stage_kernel<256,16,1>, csrc/bottleneck_wide.hip) ALONE, through the probe entry
ivosw_bneck_wide_stage_probe (include/ivosw_probe.h, libivosw_probe.so): round 7 rebuilt the body's phase B (three addresses per
(tap, slice) with the pixel tiles as immediates, zero rows at the head of six staging tiles, a second fragment register set read a
whole k-step ahead, one rolling weight set) and takes the lane id afresh in every phase, so every output element is held

  (a) to the float64 restatement of tests/bneck_ref.py at the bound tests/test_gpu_bneck_kernels.py uses for this kernel
      (|y - ref64| <= 2^-8 |ref64| + 4 d32 per element, mean |y - ref64| <= 1.5 m32), block by block: block j of a run is checked as a
      function of the input it really had (x, or the run's own y[j - 1]), with d32 = max |ref32 - ref64| of THAT block's weights over
      a batch of 8 frames (2^19 t1 values, as bneck_ref.DENSE_T1 asks) of a float64 reference chain, and m32 over the case's frames:
      both yardsticks come from the two CPU restatements alone;
  (b) bit for bit to the same blocks run one launch per block through bneck_wide_kernel<256,16,1> (chain = 0, what STAGE_RUN = 0 does
      in the tower), for the ping-pong run (every block's output) and the in-place run (first and last block's output; the buffers in
      between must stay untouched, and the first buffer ends as the output of the last in-place block).

Frames 1 / 2 / 3 (one workgroup; fewer than CUs; odd), runs of 1 / 2 / 5 blocks (first = last block; no in-place block; three in-place
blocks).  The stage kernel takes no walk direction (a workgroup is a frame), so there is no second direction to run.
Operands: x = relu(randn) per channel scale (post-ReLU statistics), weights as synth.assessnet_state_dict folds them (conv ~ N(0, 2 / fan_out),
BN gamma in [0.5, 1) - x 0.2 for the block's last BN -, running variance in [0.5, 1.5), beta and conv bias in [-0.1, 0.1)), rounded to bf16."""
import contextlib
import functools

import pytest
import torch

from ivos_w_amd import _lib as L
from tests import bneck_ref as R

pytestmark = pytest.mark.gpu

CM, CIN, H, NBLK, NREF = 256, 1024, 16, 5, 8


@functools.lru_cache(maxsize=None)
def operands():
    """x [NREF,16,16,1024] >= 0 and per block (wa, ba, wb, bb, wc, bc); everything holds bf16 values (biases fp32)."""
    g = torch.Generator().manual_seed(70256)
    r16 = lambda t: t.to(torch.bfloat16).float()
    x = r16(torch.relu(torch.randn(NREF, H, H, CIN, generator=g)) * (1 + torch.arange(CIN) % 7 * 0.25))

    def folded(cout, k, fan_out, last):
        w = torch.randn(cout, k, generator=g) * (2.0 / fan_out) ** 0.5
        gamma = (0.5 + 0.5 * torch.rand(cout, generator=g)) * (0.2 if last else 1.0)
        var, beta = 0.5 + torch.rand(cout, generator=g), 0.2 * torch.rand(cout, generator=g) - 0.1
        mean = 0.1 * torch.randn(cout, generator=g)
        s = gamma / (var + 1e-5).sqrt()
        return r16(w * s[:, None]), (beta - mean * s).float()
    blocks = []
    for _ in range(NBLK):
        wa, ba = folded(CM, CIN, CM, False)
        wb, bb = folded(CM, 9 * CM, 9 * CM, False)
        wc, bc = folded(CIN, CM, CIN, True)
        blocks.append((wa, ba, wb, bb, wc, bc))
    return x, tuple(blocks)


@functools.lru_cache(maxsize=None)
def d32_of_blocks():
    """Per block: max |ref32 - ref64| over NREF frames of the float64 reference chain (its bf16-rounded outputs feed the next block)."""
    x, blocks = operands()
    out = []
    for w in blocks:
        r64, r32 = R.ref64(x, *w), R.ref32(x, *w)
        out.append(R.bounds(r64, r32)[0])
        x = R.bf16_rne(r64).float()
    return tuple(out)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _frame_kernels():
    """The probe library with the half-frame kernel switched off (launches this small would take it block by block), put back after."""
    lib = L.probe_lib()
    try:
        assert lib.ivosw_tune_set(b"HALF16_MAX", 0) == 0
        yield lib
    finally:
        assert lib.ivosw_tune_set(b"HALF16_MAX", 96) == 0


def _device_operands(dev, n):
    _, blocks = operands()
    w = torch.cat([torch.cat([t.to(torch.bfloat16).reshape(-1) for t in (b[0], b[2], b[4])]) for b in blocks[:n]]).to(dev).contiguous()
    bias = torch.cat([torch.cat([b[1], b[3], b[5]]) for b in blocks[:n]]).float().to(dev).contiguous()
    frag = torch.full((w.numel() * 2 + 256,), 0xA5, dtype=torch.uint8, device=dev)
    frag[-256:] = 0
    return w, bias, frag


def _launch(dev, lib, B, n, chain, inplace):
    """One probe call; returns (status, int16 view of [guard frame | n x B frames | guard frame] on the CPU)."""
    x = operands()[0][:B].to(torch.bfloat16).to(dev).contiguous()
    w, bias, frag = _device_operands(dev, n)
    buf = torch.full((n * B + 2, H, H, CIN), R.NAN_BITS, dtype=torch.int16, device=dev)
    rc = lib.ivosw_bneck_wide_stage_probe(L.dptr(x), L.dptr(buf[1:]), L.dptr(w), L.dptr(bias), L.dptr(frag), n, B, chain, inplace, None,
                                          L.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, buf.cpu()


def _run(dev, lib, B, n, chain, inplace):
    rc, buf = _launch(dev, lib, B, n, chain, inplace)
    assert rc == 0, lib.ivosw_last_error().decode()
    assert bool((buf[0] == R.NAN_BITS).all()) and bool((buf[-1] == R.NAN_BITS).all()), "guard frame written"
    return buf[1:-1].reshape(n, B, H, H, CIN)


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_chained_run_matches_fp64_and_the_per_block_launches(dev, B, n):
    x, blocks = operands()
    d32 = d32_of_blocks()
    with _frame_kernels() as lib:
        chained, separate, inplace = [_run(dev, lib, B, n, c, i) for c, i in ((1, 0), (0, 0), (1, 1))]
    # (b) bit for bit: every block of the ping-pong run, first and last of the in-place run, nothing in between
    for j in range(n):
        assert torch.equal(chained[j], separate[j]), f"block {j}: chained run differs from the per-block launch"
    # (in place, y[0] is block 0's output and then the input and output of blocks 1 .. n - 2: it ends as the last of those)
    assert torch.equal(inplace[n - 1], separate[n - 1]) and torch.equal(inplace[0], separate[max(n - 2, 0)]), "in-place run differs"
    assert all(bool((inplace[j] == R.NAN_BITS).all()) for j in range(1, n - 1)), "an in-place block wrote a buffer of its own"
    # (a) every element of every block against fp64, on the input the block really had
    xin = x[:B]
    for j in range(n):
        y = chained[j].contiguous().view(torch.bfloat16).float()
        assert bool(torch.isfinite(y).all()), f"block {j}: {int((~torch.isfinite(y)).sum())} elements not written or not finite"
        r64, r32 = R.ref64(xin, *blocks[j]), R.ref32(xin, *blocks[j])
        ratio, mean, _, m32 = R.figures(y, r64, d32[j], R.bounds(r64, r32)[1])
        print(f"\nB={B} n={n} block {j}: d32 {d32[j]:.3e}  m32 {m32:.3e}  worst |y-ref64| / bound {ratio:.3f}  mean |y-ref64| {mean:.3e} = {mean / m32:.3f} m32")
        assert ratio <= 1.0, f"block {j}: an element is {ratio:.2f} x its bound (d32 {d32[j]:.3e})"
        assert mean <= 1.5 * m32, f"block {j}: mean error {mean:.3e} against m32 {m32:.3e}"
        xin = y


def test_chained_probe_refuses_what_the_tower_would_not_chain(dev):
    """Default tunables: three frames take the half-frame kernel block by block, so a chained run is refused and writes nothing."""
    lib = L.probe_lib()
    rc, buf = _launch(dev, lib, 3, 2, 1, 0)
    assert rc != 0 and "not covered" in lib.ivosw_last_error().decode()
    assert bool((buf == R.NAN_BITS).all()), "a refused call wrote y"
