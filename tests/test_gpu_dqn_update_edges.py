"""GPU: the stand-alone update entries (ivosw_clamp_adam_dev, ivosw_clamp_adam_dev_sched, ivosw_clamp_sgd, ivosw_clamp_sgd_dev_sched) at the
edges of the arena traversal they share (csrc/dqn_update.h: for_each_group): the one-element-per-lane form, every n % 4 tail, a tail in the
last lane of a workgroup and in a workgroup of its own, a workgroup that has only its ticket to take.  Three consecutive launches per case
on slices of larger buffers whose other floats hold a NaN bit pattern.  The yardsticks: ivosw_clamp_adam (the host-stepped kernel, which
dqn.hip documents as giving identical bits) on aligned copies, and torch.optim.SGD on the CPU fed the same gradients clamped on the host."""
import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L

pytestmark = pytest.mark.gpu

PAD = 64                    # floats on both sides of a slice; 256 bytes, so a slice without a shift keeps the allocation's alignment
NAN_BITS = 0x7FC0BEEF
BETA1, BETA2, EPS, WD, CLAMP, MU = 0.9, 0.999, 1e-8, 5e-4, 1.0, 0.9
LR_TABLE = np.array([1e-3, 7e-4], np.float32)       # lr_steps = 1: the three launches read entries 0, 1, 1

# (n, shift of the parameter and optimizer arrays, shift of the gradient array), in floats
SMALL = [(1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (7, 0, 0)]
# 1024 lanes: 1023 vectors + one tail element in the last lane of workgroup 0, workgroup 1 takes only its ticket; 1024 vectors, the three
# tail elements in workgroup 1; one element per lane over two workgroups, every array or only the gradient off the 16-byte grid
SHAPES_1024 = SMALL + [(4093, 0, 0), (4099, 0, 0), (1025, 1, 1), (1025, 0, 1)]
SHAPES_256 = SMALL + [(1021, 0, 0), (1027, 0, 0), (257, 1, 1), (257, 0, 1)]         # the same at ivosw_clamp_sgd's 256 lanes
ids = lambda shapes: [f"n{n}_p{s}_g{g}" for n, s, g in shapes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class Guarded:
    """n floats at PAD + shift of a buffer whose other floats are NAN_BITS."""

    def __init__(self, dev, values, shift):
        n = len(values)
        self.buf = torch.full((PAD + shift + n + PAD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.lo, self.hi = PAD + shift, PAD + shift + n
        self.x = self.buf.view(torch.float32)[self.lo:self.hi]
        self.x.copy_(torch.from_numpy(values))
        assert (self.x.data_ptr() % 16 == 0) == (shift == 0)

    def guards_intact(self):
        return bool((self.buf[:self.lo] == NAN_BITS).all()) and bool((self.buf[self.hi:] == NAN_BITS).all())


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def gradient(rng, n, k):
    g = (rng.randn(n) * 1.5).astype(np.float32)
    g[0] = 1.75 if k % 2 else -1.75                 # some exceed the clamp at every n
    assert (np.abs(g) > CLAMP).any()
    return g


def state_words(state):
    return state.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("n,shift,gshift", SHAPES_1024, ids=ids(SHAPES_1024))
@pytest.mark.parametrize("sched", [False, True], ids=["const", "sched"])
def test_clamp_adam_dev_edges(dev, n, shift, gshift, sched):
    """ivosw_clamp_adam_dev[_sched] against ivosw_clamp_adam at host step k (the scheduled entry: fed lr_table[min(k - 1, lr_steps)]) on
    aligned copies, bit for bit after each of three launches; guards untouched; then the counter (int32 at byte 16 of the Adam state)
    reads 3 and the ticket (byte 28) 0."""
    lib, st = L.lib(), L.stream_ptr(dev)
    rng = np.random.RandomState(1000 * n + 10 * shift + gshift)
    init = dict(p=(rng.randn(n) * 0.1).astype(np.float32), m=(rng.randn(n) * 0.01).astype(np.float32),
                v=(rng.rand(n) * 1e-4).astype(np.float32))
    got = {k: Guarded(dev, x, shift) for k, x in init.items()}
    ref = {k: torch.from_numpy(x).to(dev) for k, x in init.items()}
    state = torch.zeros(lib.ivosw_adam_state_bytes(), dtype=torch.uint8, device=dev)
    table = torch.from_numpy(np.append(LR_TABLE, np.float32(np.nan))).to(dev)          # a read past the table would poison the update
    for k in (1, 2, 3):
        g_np = gradient(rng, n, k)
        g, g_ref = Guarded(dev, g_np, gshift), torch.from_numpy(g_np).to(dev)
        lr = float(LR_TABLE[min(k - 1, 1)]) if sched else float(LR_TABLE[0])
        if sched:
            L.check(lib.ivosw_clamp_adam_dev_sched(L.dptr(got["p"].x), L.dptr(g.x), L.dptr(got["m"].x), L.dptr(got["v"].x), n, L.dptr(state),
                                                   L.dptr(table), 1, BETA1, BETA2, EPS, WD, CLAMP, 1.0, st), "clamp_adam_dev_sched")
        else:
            L.check(lib.ivosw_clamp_adam_dev(L.dptr(got["p"].x), L.dptr(g.x), L.dptr(got["m"].x), L.dptr(got["v"].x), n, L.dptr(state), lr,
                                             BETA1, BETA2, EPS, WD, CLAMP, 1.0, st), "clamp_adam_dev")
        L.check(lib.ivosw_clamp_adam(L.dptr(ref["p"]), L.dptr(g_ref), L.dptr(ref["m"]), L.dptr(ref["v"]), n, k, lr, BETA1, BETA2, EPS, WD, CLAMP,
                                     1.0, st), "clamp_adam")
        for name in ("p", "m", "v"):
            np.testing.assert_array_equal(bits(got[name].x), bits(ref[name]), err_msg=f"{name} after launch {k}")
            assert got[name].guards_intact(), (name, k)
        np.testing.assert_array_equal(bits(g.x), g_np.view(np.int32), err_msg=f"gradient after launch {k}")
        assert g.guards_intact(), k
        assert not np.array_equal(bits(ref["p"]), init["p"].view(np.int32))
    words = state_words(state)
    assert words[4] == 3 and words[7] == 0, words


def run_sgd(dev, n, shift, gshift, nesterov, sched):
    lib, st = L.lib(), L.stream_ptr(dev)
    rng = np.random.RandomState(1000 * n + 10 * shift + gshift + 7)
    p0 = (rng.randn(n) * 0.1).astype(np.float32)
    p, buf = Guarded(dev, p0, shift), Guarded(dev, np.zeros(n, np.float32), shift)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref = torch.optim.SGD([q], lr=float(LR_TABLE[0]), momentum=MU, dampening=0, weight_decay=WD, nesterov=nesterov, foreach=False)
    state = torch.zeros(lib.ivosw_sgd_state_bytes(), dtype=torch.uint8, device=dev)
    table = torch.from_numpy(np.append(LR_TABLE, np.float32(np.nan))).to(dev)
    for k in (1, 2, 3):
        g_np = gradient(rng, n, k)
        g = Guarded(dev, g_np, gshift)
        if sched:
            L.check(lib.ivosw_clamp_sgd_dev_sched(L.dptr(p.x), L.dptr(g.x), L.dptr(buf.x), n, L.dptr(state), L.dptr(table), 1, MU, WD,
                                                  int(nesterov), CLAMP, 1.0, st), "clamp_sgd_dev_sched")
            ref.param_groups[0]["lr"] = float(LR_TABLE[min(k - 1, 1)])
        else:
            L.check(lib.ivosw_clamp_sgd(L.dptr(p.x), L.dptr(g.x), L.dptr(buf.x), n, float(LR_TABLE[0]), MU, WD, int(nesterov), CLAMP, 1.0, st),
                    "clamp_sgd")
        q.grad = torch.from_numpy(g_np).clamp(-CLAMP, CLAMP)
        ref.step()
        np.testing.assert_array_equal(p.x.cpu().numpy(), q.detach().numpy(), err_msg=f"parameters after launch {k}")
        np.testing.assert_array_equal(buf.x.cpu().numpy(), ref.state[q]["momentum_buffer"].numpy(), err_msg=f"momentum buffer after launch {k}")
        np.testing.assert_array_equal(bits(g.x), g_np.view(np.int32), err_msg=f"gradient after launch {k}")
        assert p.guards_intact() and buf.guards_intact() and g.guards_intact(), k
    assert not np.array_equal(q.detach().numpy(), p0)
    return state_words(state)


@pytest.mark.parametrize("n,shift,gshift", SHAPES_256, ids=ids(SHAPES_256))
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_clamp_sgd_edges(dev, n, shift, gshift, nesterov):
    """ivosw_clamp_sgd (256 lanes, no counter) against torch.optim.SGD(momentum 0.9, weight_decay 5e-4) on the CPU: parameters and
    momentum buffer equal after each of three launches; guards untouched."""
    run_sgd(dev, n, shift, gshift, nesterov, sched=False)


@pytest.mark.parametrize("n,shift,gshift", SHAPES_1024, ids=ids(SHAPES_1024))
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_clamp_sgd_dev_sched_edges(dev, n, shift, gshift, nesterov):
    """ivosw_clamp_sgd_dev_sched (1024 lanes) against torch.optim.SGD with group["lr"] = lr_table[min(k - 1, lr_steps)] before step k; then
    the counter (int32 at byte 0 of the SGD state) reads 3 and the ticket (byte 4) 0."""
    words = run_sgd(dev, n, shift, gshift, nesterov, sched=True)
    assert words[0] == 3 and words[1] == 0, words
