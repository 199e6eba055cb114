"""The ragged Brain forward: K sequences, each of its own length, in one launch chain (ivosw_brain_forward_ragged,
ivosw_brain_argmax_ragged, ivosw_quality_state_ragged, Brain.forward_ragged, Agent.actions, utils_agent.recommend_frames).  Every entry is
DEFINED as equal, bit for bit, to its single-sequence counterpart per sequence, which the existing tests pin against the reference; the
forward is also held to the oracle at the tolerance test_brain_forward_vs_reference_golden holds the N = 1 path to."""
import copy
import random

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models.agent import Agent, Brain
from ivos_w_amd.models.assessment import AssessNet, pack_frames
from ivos_w_amd.utils import utils_agent

pytestmark = pytest.mark.gpu

LENGTH_SETS = {
    "one": [1],
    "two": [2],
    "ones": [1, 1, 1],
    "tiles": [1, 2, 3, 47, 48, 49, 63, 64, 65],          # R = 342: the sequences straddle the 48-row encoder / decoder tiles
    "long_short": [300, 1],                              # a one-step workgroup beside a long one
    "full_grid": [1 + k % 4 for k in range(128)],        # 128 sequences: the full 256-workgroup grid
}
SENTINEL = 64


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def P():
    return synth.brain_state_dict(0)


@pytest.fixture(scope="module")
def net(dev, P):
    b = Brain()
    b.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return b.to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(lengths, seed):
    return np.random.RandomState(seed).rand(sum(lengths), 2).astype(np.float32)


def _forward_single(net, x, T):
    """ivosw_brain_forward(N = 1, T) through the C entry."""
    lib = L.lib()
    q = torch.empty(T, dtype=torch.float32, device=x.device)
    nb = lib.ivosw_brain_ws_bytes(1, T)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=x.device)
    L.check(lib.ivosw_brain_forward(L.dptr(net.flat), L.dptr(x), 1, T, L.dptr(q), L.dptr(ws), nb, L.stream_ptr(x.device)), "brain_forward")
    return q


def _forward_ragged(net, x, lengths):
    """ivosw_brain_forward_ragged through the C entry, q with SENTINEL guard floats behind its R rows."""
    lib = L.lib()
    R = sum(lengths)
    q = torch.full((R + SENTINEL,), -7.5, dtype=torch.float32, device=x.device)
    arr = L.int_array(lengths)
    assert lib.ivosw_brain_ragged_rows(arr, len(lengths)) == R
    nb = lib.ivosw_brain_ragged_ws_bytes(R)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=x.device)
    L.check(lib.ivosw_brain_forward_ragged(L.dptr(net.flat), L.dptr(x), arr, len(lengths), L.dptr(q), L.dptr(ws), nb, L.stream_ptr(x.device)),
            "brain_forward_ragged")
    return q


@pytest.fixture(scope="module")
def ragged_runs(dev, net):
    """Per length set: the inputs, the ragged Q (with its guard floats) and the N = 1 forward of every slice - computed once, shared."""
    out = {}
    for i, (name, lengths) in enumerate(LENGTH_SETS.items()):
        xh = _inputs(lengths, 40 + i)
        x = torch.from_numpy(xh).to(dev)
        q = _forward_ragged(net, x, lengths)
        singles, off = [], 0
        for T in lengths:
            singles.append(_forward_single(net, x[off:off + T].contiguous(), T))
            off += T
        out[name] = (xh, q, singles)
    torch.cuda.synchronize(dev)
    return out


@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_ragged_forward_equals_the_single_forward_bit_for_bit(ragged_runs, name):
    lengths = LENGTH_SETS[name]
    _, q, singles = ragged_runs[name]
    R = sum(lengths)
    assert bool((q[R:] == -7.5).all())                                  # nothing written behind the last row
    want = torch.cat(singles)
    assert torch.isfinite(want).all() and (R == 1 or float(q[:R].std()) > 0)
    assert torch.equal(_bits(q[:R]), _bits(want))
    off = 0
    for T, s in zip(lengths, singles):                                  # (per slice, to name the sequence on a failure)
        assert torch.equal(_bits(q[off:off + T]), _bits(s)), (name, off, T)
        off += T


@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_ragged_forward_against_the_oracle(ragged_runs, P, name):
    from oracle import brain_oracle as bo
    lengths = LENGTH_SETS[name]
    xh, q, _ = ragged_runs[name]
    got, off = q.cpu().numpy(), 0
    for T in lengths:
        ref = bo.brain_forward(P, xh[None, off:off + T])[0]
        np.testing.assert_allclose(got[off:off + T], ref, rtol=1e-4, atol=1e-6, err_msg=f"{name}: rows {off}..{off + T}")
        off += T


def test_ragged_is_not_padding(dev, net):
    """[3, 5]: the first sequence's backward direction starts at ITS last frame.  A [1, 5] forward on the zero-padded state starts it
    two frames later, from a state the padding frames have already moved: its first three columns differ."""
    xh = _inputs([3, 5], 7)
    x = torch.from_numpy(xh).to(dev)
    q = _forward_ragged(net, x, [3, 5])[:8]
    padded = torch.zeros(5, 2, device=dev)
    padded[:3] = x[:3]
    qp = _forward_single(net, padded, 5)
    assert torch.equal(_bits(q[:3]), _bits(_forward_single(net, x[:3].contiguous(), 3)))
    assert not torch.equal(_bits(q[:3]), _bits(qp[:3]))
    assert float((q[:3] - qp[:3]).abs().max()) > 1e-6


def test_ragged_forward_refusals_launch_nothing(dev, net):
    lib, st = L.lib(), L.stream_ptr(dev)
    msg = lambda: lib.ivosw_last_error().decode()
    x = torch.rand(8, 2, device=dev)
    q = torch.full((8,), -7.5, device=dev)
    nb = lib.ivosw_brain_ragged_ws_bytes(8)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
    run = lambda arr, n, nbytes=nb: lib.ivosw_brain_forward_ragged(L.dptr(net.flat), L.dptr(x), arr, n, L.dptr(q), L.dptr(ws), nbytes, st)
    assert run(L.int_array([3, 5]), 0) == -1 and "n_seqs" in msg()
    assert run(L.int_array([2] * 129), 129) == -1 and "n_seqs" in msg()
    assert run(L.int_array([3, 0, 5]), 3) == -1 and "sequence 1" in msg()
    assert run(L.int_array([1 << 20, 1]), 2) == -1 and "sequence 1" in msg() and "2^20" in msg()
    assert run(L.int_array([3, 5]), 2, 16) == -2 and "workspace" in msg()
    torch.cuda.synchronize(dev)
    assert bool((q == -7.5).all())
    assert run(L.int_array([3, 5]), 2) == 0
    torch.cuda.synchronize(dev)
    assert bool((q != -7.5).all())


# ---------------------------------------------------------------------------------------------- workspaces of exactly the reported size
GUARD = 1 << 20     # bytes of pattern behind the exact-size workspace: allocated memory, so a miscounted workspace shows and cannot fault


def _exact_and_roomy(dev, nb, run):
    """run(ws, nbytes) -> output tensors: once in a workspace of exactly the nb reported bytes, cut from a larger tensor whose rest holds a
    byte pattern, once in a generously oversized one.  The outputs are bit-equal and the pattern is untouched."""
    nb = int(nb)
    assert nb > 0 and nb % 256 == 0
    buf = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    exact = run(buf[:nb], nb)
    torch.cuda.synchronize(dev)
    assert bool((buf[nb:] == 0xA5).all()), "the bytes behind the exact-size workspace were written"
    big = torch.full((2 * nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    roomy = run(big, big.numel())
    torch.cuda.synchronize(dev)
    assert len(exact) == len(roomy)
    for a, b in zip(exact, roomy):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("N,T", [(1, 1), (3, 7)])
def test_brain_forward_in_a_workspace_of_exactly_the_reported_size(dev, net, N, T):
    lib, st = L.lib(), L.stream_ptr(dev)
    x = torch.from_numpy(_inputs([N * T], 70 + N)).to(dev)

    def run(ws, nbytes):
        q = torch.full((N * T,), -7.5, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_brain_forward(L.dptr(net.flat), L.dptr(x), N, T, L.dptr(q), L.dptr(ws), nbytes, st), "brain_forward")
        return (q,)
    _exact_and_roomy(dev, lib.ivosw_brain_ws_bytes(N, T), run)


def test_ragged_forward_in_a_workspace_of_exactly_the_reported_size(dev, net):
    lib, st = L.lib(), L.stream_ptr(dev)
    lengths = [1, 5, 2]
    x, arr = torch.from_numpy(_inputs(lengths, 75)).to(dev), L.int_array(lengths)

    def run(ws, nbytes):
        q = torch.full((sum(lengths),), -7.5, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_brain_forward_ragged(L.dptr(net.flat), L.dptr(x), arr, len(lengths), L.dptr(q), L.dptr(ws), nbytes, st), "forward_ragged")
        return (q,)
    _exact_and_roomy(dev, lib.ivosw_brain_ragged_ws_bytes(sum(lengths)), run)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (5, 25)])
def test_dqn_loss_grad_in_a_workspace_of_exactly_the_reported_size(dev, net, B, T):
    """(1, 1) and (3, 2) take the un-fused two-stream chain (a pass of fewer than eight rows), (5, 25) the fused one."""
    lib, st = L.lib(), L.stream_ptr(dev)
    tgt = Brain()
    tgt.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(1).items()})
    tgt = tgt.to(dev)
    g = torch.Generator().manual_seed(100 * B + T)
    state, new_state = (torch.rand(B, T, 2, generator=g).to(dev) for _ in range(2))
    action = torch.randint(0, T, (B,), generator=g).to(dev)
    r_step, r_done = (torch.rand(B, generator=g).to(dev) for _ in range(2))

    def run(ws, nbytes):
        grads = torch.zeros(L.BRAIN_NPARAMS, dtype=torch.float32, device=dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_dqn_loss_grad_ex(L.dptr(net.flat), L.dptr(tgt.flat), L.dptr(state), L.dptr(new_state), L.dptr(action), L.dptr(r_step),
                                           L.dptr(r_done), B, T, 0.95, L.DQN_LOSS_MSE, 1.0, L.dptr(grads), L.dptr(loss), L.dptr(ws), nbytes, st),
                "dqn_loss_grad_ex")
        return grads, loss
    _exact_and_roomy(dev, lib.ivosw_dqn_ws_bytes(B, T), run)


# ---------------------------------------------------------------------------------------------- argmax
def test_argmax_ragged_is_the_first_maximum_per_sequence(dev):
    lib, st = L.lib(), L.stream_ptr(dev)
    lengths = [1, 2, 63, 64, 65, 130]
    rs = np.random.RandomState(3)
    rows = [rs.rand(n).astype(np.float32) for n in lengths]
    rows[1][:] = 0.25                                                   # all equal: index 0
    rows[2][[17, 40]] = 2.0                                             # two equal maxima: the first wins
    rows[3][63] = 3.0                                                   # the maximum in the last column
    rows[4][[64, 0]] = 4.0                                              # equal maxima in the first and the last column (the second lane round)
    rows[5][[129, 70]] = 5.0                                            # equal maxima in the second and third round of one lane pair
    flat = torch.from_numpy(np.concatenate(rows)).to(dev)
    want = [int(np.argmax(r)) for r in rows]
    assert want == [0, 0, 17, 63, 0, 70]
    idx = torch.full((len(lengths) + 1,), -1, dtype=torch.int64, device=dev)
    L.check(lib.ivosw_brain_argmax_ragged(L.dptr(flat), L.int_array(lengths), len(lengths), L.dptr(idx), st), "argmax_ragged")
    single, off = [], 0
    for n in lengths:
        one = torch.full((1,), -1, dtype=torch.int64, device=dev)
        L.check(lib.ivosw_brain_argmax(L.dptr(flat[off:off + n]), 1, n, L.dptr(one), st), "argmax")
        single.append(int(one.cpu()[0]))
        off += n
    got = idx.cpu().tolist()
    assert got[:-1] == want == single and got[-1] == -1
    # all-equal rows of every length
    flat.fill_(1.5)
    L.check(lib.ivosw_brain_argmax_ragged(L.dptr(flat), L.int_array(lengths), len(lengths), L.dptr(idx), st), "argmax_ragged")
    assert idx.cpu().tolist() == [0] * len(lengths) + [-1]


# ---------------------------------------------------------------------------------------------- quality -> state
def test_quality_state_ragged_equals_quality_state_per_video(dev):
    lib, st = L.lib(), L.stream_ptr(dev)
    n_obj, lengths = [1, 7, 8, 9, 17], [1, 5, 64, 65, 3]
    R, units = sum(lengths), sum(o * n for o, n in zip(n_obj, lengths))
    g = torch.Generator().manual_seed(21)
    scores = torch.rand(units, generator=g).to(dev)
    counts = torch.randint(0, 4, (R,), generator=g).float().to(dev)
    quality = torch.full((R + 1,), -1.0, dtype=torch.float64, device=dev)
    state = torch.full((R + 1, 2), -1.0, dtype=torch.float32, device=dev)
    L.check(lib.ivosw_quality_state_ragged(L.dptr(scores), L.int_array(n_obj), L.int_array(lengths), len(lengths), L.dptr(counts),
                                           L.dptr(quality), L.dptr(state), st), "quality_state_ragged")
    u = r = 0
    for o, n in zip(n_obj, lengths):
        qk = torch.empty(n, dtype=torch.float64, device=dev)
        sk = torch.empty(n, 2, dtype=torch.float32, device=dev)
        L.check(lib.ivosw_quality_state(L.dptr(scores[u:u + o * n]), o, n, L.dptr(counts[r:r + n]), L.dptr(qk), L.dptr(sk), st), "quality_state")
        assert torch.equal(quality[r:r + n].view(torch.int64), qk.view(torch.int64)), (o, n)
        assert torch.equal(_bits(state[r:r + n]), _bits(sk)), (o, n)
        u += o * n
        r += n
    assert float(quality[R]) == -1.0 and bool((state[R] == -1.0).all()) and float(quality[:R].std()) > 0


# ---------------------------------------------------------------------------------------------- Python: grouping, tunables
def test_forward_ragged_groups_more_than_128_sequences(dev, net):
    lengths = [1 + k % 3 for k in range(130)]
    x = torch.from_numpy(_inputs(lengths, 77)).to(dev)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    states = [x[int(o):int(o) + n] for o, n in zip(offs[:-1], lengths)]
    q, views = net.forward_ragged(states)
    assert q.shape == (sum(lengths),) and [v.shape[0] for v in views] == lengths
    q2, _ = net.forward_ragged(x, lengths)                              # the flat form
    q3, _ = net.forward_ragged([s.clone() for s in states])             # separate tensors: concatenated
    for k, (s, v) in enumerate(zip(states, views)):
        assert torch.equal(_bits(v), _bits(net(s[None])[0])), k
    assert torch.equal(_bits(q), _bits(q2)) and torch.equal(_bits(q), _bits(q3)) and float(q.std()) > 0


def test_ragged_forward_with_the_quad_recurrence_switched_off(dev, net):
    lengths = [3, 49, 1, 20]
    x = torch.from_numpy(_inputs(lengths, 11)).to(dev)
    L.tune_set("LSTM_QUAD", 0)
    try:
        q = _forward_ragged(net, x, lengths)
        singles, off = [], 0
        for T in lengths:
            singles.append(_forward_single(net, x[off:off + T].contiguous(), T))
            off += T
        torch.cuda.synchronize(dev)
    finally:
        L.tune_set("LSTM_QUAD", 1)
    R = sum(lengths)
    assert torch.equal(_bits(q[:R]), _bits(torch.cat(singles))) and bool((q[R:] == -7.5).all()) and float(q[:R].std()) > 0


# ---------------------------------------------------------------------------------------------- recommend_frames
class _Vid:
    def __init__(self, frames, all_P, O, n):
        self.frames, self.all_P, self.O, self.n = frames, all_P, O, n


def _random_video(dev, g, n, O, H, W, u8=False):
    if u8:
        frames = pack_frames(torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8), dev)
    else:
        frames = torch.rand(n, 3, H, W, generator=g).to(dev)
    return _Vid(frames, torch.rand(n, O + 1, H, W, generator=g).to(dev), O, n)


@pytest.fixture(scope="module")
def assess(dev):
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()}, strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("phase,seed", [("eval", 3), ("train", 2)])
def test_recommend_frames_is_one_ragged_chain(dev, assess, monkeypatch, capsys, phase, seed):
    cfg = AD(phase=phase, data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                          update_rate=0.05, lr=5e-6, weight_decay=5e-4))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    twin = copy.deepcopy(agent)
    g = torch.Generator().manual_seed(99)
    vids = [_random_video(dev, g, 6, 2, 24, 36), _random_video(dev, g, 4, 1, 31, 27, u8=True), _random_video(dev, g, 9, 3, 18, 40)]

    def requests():
        return [dict(n_frame=v.n, n_objects=v.O, all_F=v.frames, all_P=v.all_P, new_masks_quality=np.zeros(v.n), prev_frames=[1],
                     annotated_frames_list=[1, 1, 0], mask_quality=np.zeros(v.n), first_frame=1, max_nb_interactions=8) for v in vids]
    cy = AD(setting="wild", method="ours")
    utils_agent.clear_frame_cache()
    random.seed(seed)
    np.random.seed(seed)
    want_req = requests()
    want = [int(utils_agent.recommend_frame(cy, assess, twin, dev, **r)) for r in want_req]
    log_want = capsys.readouterr().out
    rng_want = (random.random(), float(np.random.rand()))
    if phase == "train":                                                # the seed mixes both branches
        assert 0 < log_want.count("randomly") < 3 and log_want.count("by agent") == 3 - log_want.count("randomly")
    else:
        assert log_want.count("by agent") == 3
    random.seed(seed)
    np.random.seed(seed)
    got_req = requests()
    calls = []
    real_cpu, real_item, real_fwd, real_ragged = torch.Tensor.cpu, torch.Tensor.item, Brain.forward, Brain.forward_ragged
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(Brain, "forward", lambda self, *a, **k: (calls.append("forward"), real_fwd(self, *a, **k))[1])
    monkeypatch.setattr(Brain, "forward_ragged", lambda self, *a, **k: (calls.append("forward_ragged"), real_ragged(self, *a, **k))[1])
    got = [int(i) for i in utils_agent.recommend_frames(cy, assess, agent, dev, got_req)]
    monkeypatch.undo()
    assert sorted(calls) == ["cpu", "forward_ragged"], calls            # ONE ragged forward, ONE device-to-host copy, no Brain.forward
    assert got == want and all(0 <= i < v.n for i, v in zip(got, vids))
    for a, b in zip(got_req, want_req):
        np.testing.assert_array_equal(a["mask_quality"], b["mask_quality"])
        assert np.ptp(a["mask_quality"]) > 0
    assert capsys.readouterr().out == log_want
    assert agent.steps_done == twin.steps_done == 3
    assert (random.random(), float(np.random.rand())) == rng_want       # the host RNG streams moved as under sequential calls
    utils_agent.clear_frame_cache()
