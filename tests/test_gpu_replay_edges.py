"""The replay kernels of csrc/dqn.hip at their edges, through the C ABI, against references that do not share their arithmetic
(oracle/per_cases.py, pinned on the CPU by tests/test_oracle_per_cases.py):

  a. ivosw_per_build          carried leaves bit-equal, new ones 2 ulp from float64, padding 0, no NaN left, nodes = a rebuild
  b. ivosw_per_draw_gather    rows equal to the exact model on integer-leaf trees across the three staging regimes of the draw
                              (all LDS, leaves global, several global levels) and the wave tails of B; points that sit exactly
                              on a running sum; the rounded-up last slot;
                              float trees against the mirror; a heavy and a 2^-20 leaf both drawn; weights against float64; beta and the counter's wrap; the gather
  c. ivosw_per_update         every pattern of the touched-node list against the update model on the device's own leaves
  d. ivosw_replay_draw_gather against draw_indices and numpy indexing, the counter's wrap; ivosw_replay_draw_index at n = 2^31 - 1
  e. ivosw_dqn_step_drawn     the copy of the uniform draw + gather inside the encoder launch, equal to d.

Every output lies in a buffer with 64 sentinel elements on either side, checked after the call.

Weights: |w - w64| <= 3 * max|w32 - w64| + 2^-24 per case, w32 = the same expression in float32 numpy (pc.weights32): the factor is the seg
epilogue's (a float32 evaluation in another order of operations, with another powf, may be a small multiple of numpy's distance from
float64, not an order of magnitude); the measured ratios are in LAB_NOTES.md.
"""
import functools

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models import momory_pool as mp
from oracle import per_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 64
SENTINEL = {torch.float32: -12345.0, torch.int64: -0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
WEIGHT_FACTOR = 3.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Guarded:
    """A contiguous device array with MARGIN sentinel elements on either side."""

    def __init__(self, dev, shape, dtype, fill=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        m = int(np.prod(shape))
        self.full = torch.full((m + 2 * MARGIN,), SENTINEL[dtype], dtype=dtype, device=dev)
        self.t = self.full[MARGIN:MARGIN + m].view(shape)
        if fill is not None:
            self.t.fill_(fill)
        self.m = m

    def intact(self):
        s = SENTINEL[self.full.dtype]
        return bool((self.full[:MARGIN] == s).all()) and bool((self.full[MARGIN + self.m:] == s).all())

    def np(self):
        return self.t.cpu().numpy()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ---------------------------------------------------------------- replay columns: a distinct value per (row, t, column)
@functools.lru_cache(maxsize=None)
def columns_np(n, T):
    assert n * T < 2 ** 22
    k = np.arange(n * T, dtype=np.float32).reshape(n, T)
    r = np.arange(n)
    return dict(old_iou=k, new_iou=k + np.float32(2 ** 22), ann=k + np.float32(2 ** 23), nann=k + np.float32(3 * 2 ** 22),
                action=(r * 7 + 1).astype(np.int64), rstep=(r + 0.25).astype(np.float32), rdone=(-r - 0.5).astype(np.float32))


_COLS = {}


def columns(dev, n, T):
    if (n, T) not in _COLS:
        if len(_COLS) > 8:
            _COLS.clear()
        _COLS[(n, T)] = {k: torch.from_numpy(v).to(dev) for k, v in columns_np(n, T).items()}
    return _COLS[(n, T)]


def col_args(c):
    return [L.dptr(c[k]) for k in ("old_iou", "new_iou", "ann", "nann", "action", "rstep", "rdone")]


class Batch:
    """The guarded outputs of a draw + gather."""

    def __init__(self, dev, B, T, weights=False):
        self.idx = Guarded(dev, B, torch.int64)
        self.state, self.new_state = Guarded(dev, (B, T, 2), torch.float32), Guarded(dev, (B, T, 2), torch.float32)
        self.action = Guarded(dev, B, torch.int64)
        self.rstep, self.rdone = Guarded(dev, B, torch.float32), Guarded(dev, B, torch.float32)
        self.weights = Guarded(dev, B, torch.float32) if weights else None

    def outs(self):
        return [g for g in (self.idx, self.weights, self.state, self.new_state, self.action, self.rstep, self.rdone) if g is not None]

    def assert_gathered(self, n, T, rows, why):
        """Everything but the rows themselves: numpy indexing of the columns, bit for bit, and the margins."""
        c = columns_np(n, T)
        np.testing.assert_array_equal(self.state.np(), np.stack([c["old_iou"][rows], c["ann"][rows]], -1), err_msg=f"{why}: state")
        np.testing.assert_array_equal(self.new_state.np(), np.stack([c["new_iou"][rows], c["nann"][rows]], -1), err_msg=f"{why}: new_state")
        np.testing.assert_array_equal(self.action.np(), c["action"][rows], err_msg=f"{why}: action")
        np.testing.assert_array_equal(self.rstep.np(), c["rstep"][rows], err_msg=f"{why}: reward_step")
        np.testing.assert_array_equal(self.rdone.np(), c["rdone"][rows], err_msg=f"{why}: reward_done")
        assert all(g.intact() for g in self.outs()), f"{why}: a margin was written"


# ---------------------------------------------------------------- prioritized replay: state, tree, calls
def per_state(dev, seed, counter, max_priority=1.0):
    raw = np.zeros(4, np.uint64)
    raw[0] = np.uint64(seed)
    raw[1] = np.uint64(counter & 0xFFFFFFFF)
    raw[2] = np.uint64(np.array([max_priority], np.float32).view(np.uint32)[0])
    g = Guarded(dev, 32, torch.uint8)
    g.t.copy_(torch.from_numpy(raw.view(np.uint8).copy()))
    assert L.lib().ivosw_per_state_bytes() == 32
    return g


def state_fields(g):
    raw = g.np()
    return int(raw[0:8].view(np.uint64)[0]), int(raw[8:12].view(np.uint32)[0]), raw[16:20].view(np.float32)[0]


def build_tree(dev, n, leaves, st, alpha=0.6, n_old=None):
    """ivosw_per_build into a NaN-filled guarded tree, carrying leaves[:n_old] over (n_old = n by default)."""
    n_old = n if n_old is None else n_old
    tree = Guarded(dev, int(L.lib().ivosw_per_tree_floats(n)), torch.float32, fill=float("nan"))
    old = torch.from_numpy(np.ascontiguousarray(leaves[:n_old], np.float32)).to(dev) if n_old else None
    L.check(L.lib().ivosw_per_build(L.dptr(tree.t), n, L.dptr(old) if n_old else None, n_old, L.dptr(st.t), float(np.float32(alpha)),
                                    L.stream_ptr(dev)), "per_build")
    return tree


def per_draw(dev, n, B, T, tree, st, beta0, N):
    out = Batch(dev, B, T, weights=True)
    L.check(L.lib().ivosw_per_draw_gather(*col_args(columns(dev, n, T)), L.dptr(tree.t), L.dptr(st.t), n, B, T, float(np.float32(beta0)), N,
                                          L.dptr(out.idx.t), L.dptr(out.weights.t), L.dptr(out.state.t), L.dptr(out.new_state.t),
                                          L.dptr(out.action.t), L.dptr(out.rstep.t), L.dptr(out.rdone.t), L.stream_ptr(dev)), "per_draw_gather")
    return out


def assert_weights(why, w, leaves, root, rows, beta0, N, c):
    w64, w32 = pc.weights64(leaves, rows, beta0, N, c), pc.weights32(leaves, root, rows, beta0, N, c)
    err, err32 = np.abs(w.astype(np.float64) - w64).max(), np.abs(w32.astype(np.float64) - w64).max()
    print(f"weights {why}: kernel {err:.3e} numpy-float32 {err32:.3e} ratio to the bar's variable part {err / max(err32, 2.0 ** -24):.2f}")
    assert np.all(w > 0) and np.all(w <= 1) and w.max() == 1.0, why
    assert err <= WEIGHT_FACTOR * err32 + 2.0 ** -24, (why, err, err32)
    if float(np.float32(beta0)) == 0.0:
        assert np.all(w == 1.0), why


# ---------------------------------------------------------------- a. build
BUILD_NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 65536, 65537]


@pytest.mark.parametrize("n,n_old", [(n, k) for n in BUILD_NS for k in sorted({0, 1, n - 1, n})])
def test_build(dev, n, n_old):
    alpha, mxp = 0.6, 2.5
    rs = np.random.RandomState(n + 7 * n_old)
    old = np.ldexp(rs.uniform(0.5, 1.0, n), rs.randint(-30, 30, n)).astype(np.float32)
    st = per_state(dev, 11, 5, mxp)
    before = st.np().copy()
    tree = build_tree(dev, n, old, st, alpha, n_old)
    t = tree.np()
    P = pc.tree_leaves(n)
    assert t.shape == (2 * P,) and tree.intact() and st.intact()
    assert not np.isnan(t).any() and t[0] == 0
    assert np.array_equal(bits(t[P:P + n_old]), bits(old[:n_old])), "carried leaves"
    new = t[P + n_old:P + n]
    assert np.all(ulps(new, np.float64(np.float32(mxp)) ** np.float64(np.float32(alpha))) <= 2), "new leaves"
    assert np.all(t[P + n:] == 0), "padding"
    assert np.array_equal(bits(t), bits(mp.per_rebuild(t))) and np.array_equal(bits(t), bits(pc.rebuild(t[P:], P))), "internal nodes"
    np.testing.assert_array_equal(st.np(), before)                     # the build reads the state only


# ---------------------------------------------------------------- b. prioritized draw
DRAW_NS = [1, 2, 3, 1000, 1024, 1025, 2048, 2049, 5000]
DRAW_BS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("B", DRAW_BS)
@pytest.mark.parametrize("n", DRAW_NS)
def test_draw_rows_equal_the_exact_model(dev, n, B):
    """Integer leaves: counters 0xFFFFFFFE, 0xFFFFFFFF and 0 in three consecutive draws.  Rows, gather, weights, counter, tree."""
    T, seed, beta0, N = 2, 0xABCDEF + n, 0.4, 40
    lv = pc.int_leaves(n, B)
    st = per_state(dev, seed, 0xFFFFFFFE)
    tree = build_tree(dev, n, lv, st)
    t0 = tree.np()
    assert np.array_equal(bits(t0), bits(pc.rebuild(lv))) and t0[1] == lv.sum()
    for c in (0xFFFFFFFE, 0xFFFFFFFF, 0):
        out = per_draw(dev, n, B, T, tree, st, beta0, N)
        rows = out.idx.np()
        np.testing.assert_array_equal(rows, pc.exact_draw_rows(lv, seed, c, B), err_msg=f"counter {c:#x}")
        assert np.all(lv[rows] > 0)
        out.assert_gathered(n, T, rows, f"counter {c:#x}")
        assert_weights(f"int n={n} B={B} c={c:#x}", out.weights.np(), lv, t0[1], rows, beta0, N, c)
        assert state_fields(st) == (seed, (c + 1) & 0xFFFFFFFF, np.float32(1.0)) and st.intact()
    assert np.array_equal(bits(tree.np()), bits(t0)) and tree.intact()            # the draw reads the tree only


@pytest.mark.parametrize("front", [0, 2000])
def test_draw_points_on_the_running_sums(dev, front):
    """x == left child at some level for more than a hundred slots (pc.boundary_leaves): the walk goes right there, past zero leaves too.
    front = 0: all of the tree in LDS; 2000 zero leaves first: P = 4096, two global levels."""
    seed, c, B, T = 17, 4, 1024, 1
    lv, on = pc.boundary_leaves(seed, c, front)
    n = len(lv)
    st = per_state(dev, seed, c)
    tree = build_tree(dev, n, lv, st)
    out = per_draw(dev, n, B, T, tree, st, 0.4, 0)
    rows = out.idx.np()
    want = pc.exact_draw_rows(lv, seed, c, B)
    np.testing.assert_array_equal(rows[on], want[on], err_msg="slots whose point is a running sum")
    np.testing.assert_array_equal(rows, want)
    assert np.all(lv[rows] > 0)
    out.assert_gathered(n, T, rows, "points on the running sums")
    assert_weights(f"boundary front={front}", out.weights.np(), lv, tree.np()[1], rows, 0.4, 0, c)


@pytest.mark.parametrize("n", [1000, 1024])
def test_rounded_up_last_slot_lands_on_the_last_row(dev, n):
    """float32(1023 + u) == 1024: slot 1023 walks with x == total, right at every level, to leaf P - 1 = 1023: the last row through the
    clamp at n = 1000, through the last leaf itself at n = 1024."""
    seed, c = pc.rounded_up_slot()
    B, T = 1024, 1
    lv = pc.int_leaves(n, B)
    assert pc.draw_points(lv.sum(), seed, c, B)[B - 1] == lv.sum()
    st = per_state(dev, seed, c)
    tree = build_tree(dev, n, lv, st)
    out = per_draw(dev, n, B, T, tree, st, 0.4, 0)
    rows = out.idx.np()
    assert rows[B - 1] == n - 1
    np.testing.assert_array_equal(rows, pc.exact_draw_rows(lv, seed, c, B))
    out.assert_gathered(n, T, rows, "rounded-up slot")
    assert_weights(f"rounded-up n={n}", out.weights.np(), lv, tree.np()[1], rows, 0.4, 0, c)


@pytest.mark.parametrize("B", [1, 65, 1024])
@pytest.mark.parametrize("n", [1000, 2048, 5000])
@pytest.mark.parametrize("kind", ["hot", "wide"])
def test_draw_on_float_trees_equals_the_mirror(dev, kind, n, B):
    T, seed = 1, 99
    lv = pc.hot_leaves(n) if kind == "hot" else pc.wide_leaves(n)
    st = per_state(dev, seed, 3)
    tree = build_tree(dev, n, lv, st)
    t0 = tree.np()
    assert np.array_equal(bits(t0), bits(pc.rebuild(lv)))
    for c in (3, 4):
        out = per_draw(dev, n, B, T, tree, st, 0.4, 40)
        rows = out.idx.np()
        np.testing.assert_array_equal(rows, mp.per_draw_rows(t0, seed, c, B, n), err_msg=f"counter {c}")
        assert rows.min() >= 0 and rows.max() < n and np.all(lv[rows] > 0)
        out.assert_gathered(n, T, rows, f"counter {c}")
        assert_weights(f"{kind} n={n} B={B} c={c}", out.weights.np(), lv, t0[1], rows, 0.4, 40, c)
    if kind == "hot" and B > 1:
        assert np.all(rows[1:] == n // 3)


@pytest.mark.parametrize("beta0,N", [(0.4, 0), (0.4, 40), (1.0, 0)])
@pytest.mark.parametrize("c", [3, 4])
def test_draw_weights_on_a_heavy_and_a_light_leaf(dev, c, beta0, N):
    """pc.hot_pair_leaves: half of the mass on the last row, 2^-20 of it on a leaf under slot 100's point - both drawn, the weights a
    factor 2^(19 beta) apart (the hot-leaf trees above draw one row only: all their weights are 1)."""
    seed, B, T = 99, 1024, 1
    lv, light = pc.hot_pair_leaves(seed, c)
    n = len(lv)
    st = per_state(dev, seed, c)
    tree = build_tree(dev, n, lv, st)
    out = per_draw(dev, n, B, T, tree, st, beta0, N)
    rows = out.idx.np()
    np.testing.assert_array_equal(rows, pc.exact_draw_rows(lv, seed, c, B))
    assert rows[100] == light and (rows == n - 1).sum() == 512
    w = out.weights.np()
    assert w[100] == 1.0 and w.min() == w[B - 1] < 2.0 ** -7
    assert_weights(f"pair beta0={beta0} N={N} c={c}", w, lv, tree.np()[1], rows, beta0, N, c)
    out.assert_gathered(n, T, rows, "heavy and light leaf")


# At beta == 1 (c >= N) the weights of the power-of-two leaves are powers of two and numpy's float32 power(x, -1) is exact there, so the bar
# is its 2^-24 floor alone: (0.4, 40, 41) was measured at one ulp of a weight in [0.5, 1), 0.996 of the bar.  A powf that moves by one more
# ulp on such a weight fails this case with no defect in the kernel: read a failure here against the device library's powf first.
@pytest.mark.parametrize("beta0,N,c", [(0.4, 0, 7), (0.4, 40, 0), (0.4, 40, 39), (0.4, 40, 40), (0.4, 40, 41), (1, 5, 0), (0.4, 40, 0xFFFFFFFF),
                                       (0.0, 0, 3), (0.0, 40, 0)])
def test_draw_beta_and_counter(dev, beta0, N, c):
    """beta of draw c against float64 through the weights, on leaves a factor 2^12 apart (a beta off by one step of 40 moves the smallest
    weight by 12 %); beta0 = 0: every weight 1.  From 0xFFFFFFFF the draw uses beta(N) and leaves the counter at 0."""
    n, B, T, seed = 1000, 64, 1, 5
    lv = pc.beta_leaves(n, B)
    st = per_state(dev, seed, c)
    tree = build_tree(dev, n, lv, st)
    out = per_draw(dev, n, B, T, tree, st, beta0, N)
    rows = out.idx.np()
    np.testing.assert_array_equal(rows, pc.exact_draw_rows(lv, seed, c, B))
    assert len(np.unique(lv[rows])) >= 4
    assert_weights(f"beta0={beta0} N={N} c={c:#x}", out.weights.np(), lv, tree.np()[1], rows, beta0, N, c)
    if pc.beta64(beta0, N, c) == 1.0:                                   # fully annealed: w = smallest drawn leaf / leaf
        np.testing.assert_allclose(out.weights.np().astype(np.float64), lv[rows].min() / lv[rows], rtol=1e-6)
    assert state_fields(st)[1] == (c + 1) & 0xFFFFFFFF
    out.assert_gathered(n, T, rows, "beta")


@pytest.mark.parametrize("B", [1024, 1])
@pytest.mark.parametrize("T", [1, 2, 25, 300])
def test_per_gather(dev, T, B):
    n, seed = 1000, 21
    lv = pc.int_leaves(n, B, seed=1)
    st = per_state(dev, seed, 0)
    tree = build_tree(dev, n, lv, st)
    t0 = tree.np()
    out = per_draw(dev, n, B, T, tree, st, 0.4, 0)
    rows = out.idx.np()
    np.testing.assert_array_equal(rows, pc.exact_draw_rows(lv, seed, 0, B))
    out.assert_gathered(n, T, rows, f"T={T} B={B}")
    assert np.array_equal(bits(tree.np()), bits(t0)) and tree.intact() and st.intact()


# ---------------------------------------------------------------- c. update
def run_update(dev, n, idx, td, alpha, eps, why):
    rs = np.random.RandomState(n)
    lv = rs.uniform(0.01, 3.0, n).astype(np.float32)
    st = per_state(dev, 1, 9, 1.0)
    tree = build_tree(dev, n, lv, st, alpha)
    before = tree.np()
    P = pc.tree_leaves(n)
    assert np.array_equal(bits(before), bits(pc.rebuild(lv)))
    B = len(idx)
    d_idx, d_td = torch.from_numpy(np.asarray(idx, np.int64)).to(dev), torch.from_numpy(np.asarray(td, np.float32)).to(dev)
    L.check(L.lib().ivosw_per_update(L.dptr(tree.t), n, L.dptr(st.t), L.dptr(d_idx), L.dptr(d_td), B, float(np.float32(alpha)),
                                     float(np.float32(eps)), L.stream_ptr(dev)), "per_update")
    t = tree.np()
    assert tree.intact() and st.intact(), why
    win = pc.update_winners(idx, n)
    want_leaf = pc.update_leaf64(td, eps, alpha)
    for r, b in win.items():
        assert ulps(t[P + r], want_leaf[b]) <= 2, (why, "leaf of row", r, "slot", b, t[P + r], want_leaf[b])
    untouched = np.setdiff1d(np.arange(P), list(win))
    assert np.array_equal(bits(t[P + untouched]), bits(before[P + untouched])), f"{why}: an untouched leaf changed"
    new = np.zeros(B, np.float32)
    for r, b in win.items():
        new[b] = t[P + r]
    model = pc.update_model(before, n, idx, new)
    bad = np.flatnonzero(bits(t) != bits(model))
    assert bad.size == 0, (why, "nodes", bad[:8].tolist(), t[bad[:8]].tolist(), model[bad[:8]].tolist())
    if not win:
        assert np.array_equal(bits(t), bits(before)), why
    seed, counter, mx = state_fields(st)
    assert (seed, counter) == (1, 9) and mx == pc.update_max_priority(1.0, td, eps), (why, mx)
    return t, mx


def _patterns():
    out = []
    for n in (1, 2, 3, 50, 4096):
        out += [(n, name) for name in pc.update_patterns(n)]
    return out


@pytest.mark.parametrize("n,name", _patterns())
def test_update_patterns(dev, n, name):
    idx = pc.update_patterns(n)[name]
    td = np.random.RandomState(len(idx) + n).uniform(0, 3, len(idx)).astype(np.float32)
    td[len(idx) // 2] = 3.5                                       # the maximum sits on some slot, skipped or not: max_priority rises
    _, mx = run_update(dev, n, idx, td, 0.7, 1e-3, f"n={n} {name}")
    assert mx == np.float32(3.5) + np.float32(1e-3)


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.7])
@pytest.mark.parametrize("tdk", ["zero", "huge", "mixed"])
@pytest.mark.parametrize("n,name", [(3, "first_and_last"), (50, "random_with_repeats"), (4096, "run1_shuffled"), (4096, "one_row_everywhere")])
def test_update_values(dev, n, name, tdk, alpha):
    """td = 0 (p = eps), td = 1e30, and both among ordinary values, at alpha 0, 1 and 0.7."""
    idx = pc.update_patterns(n)[name]
    B = len(idx)
    td = {"zero": np.zeros(B), "huge": np.full(B, 1e30), "mixed": np.random.RandomState(B).uniform(0, 3, B)}[tdk].astype(np.float32)
    if tdk == "mixed":
        td[::5], td[B - 1] = 0, 1e30
    t, mx = run_update(dev, n, idx, td, alpha, 1e-6, f"n={n} {name} td={tdk} alpha={alpha}")
    assert np.isfinite(t).all()
    if alpha == 0:
        assert np.all(t[pc.tree_leaves(n) + np.array(sorted(pc.update_winners(idx, n)))] == 1.0)


# ---------------------------------------------------------------- d. uniform draw
def draw_state(dev, seed, counter):
    raw = np.zeros(2, np.uint64)
    raw[0], raw[1] = np.uint64(seed), np.uint64(counter & 0xFFFFFFFF)
    assert L.lib().ivosw_replay_draw_state_bytes() == 16
    g = Guarded(dev, 16, torch.uint8)
    g.t.copy_(torch.from_numpy(raw.view(np.uint8).copy()))
    return g


def uniform_draw(dev, n, B, T, ds):
    out = Batch(dev, B, T)
    L.check(L.lib().ivosw_replay_draw_gather(*col_args(columns(dev, n, T)), L.dptr(ds.t), n, B, T, L.dptr(out.idx.t), L.dptr(out.state.t),
                                             L.dptr(out.new_state.t), L.dptr(out.action.t), L.dptr(out.rstep.t), L.dptr(out.rdone.t),
                                             L.stream_ptr(dev)), "replay_draw_gather")
    return out


@pytest.mark.parametrize("T", [1, 25, 300])
@pytest.mark.parametrize("B", [1, 5, 129, 1025])
@pytest.mark.parametrize("n", [1, 2, 3, 500])
def test_uniform_draw(dev, n, B, T):
    seed = 0x1234_5678_9ABC_DEF0
    ds = draw_state(dev, seed, 0xFFFFFFFE)
    for c in (0xFFFFFFFE, 0xFFFFFFFF, 0):
        out = uniform_draw(dev, n, B, T, ds)
        rows = out.idx.np()
        np.testing.assert_array_equal(rows, mp.draw_indices(seed, c, B, n), err_msg=f"counter {c:#x}")
        out.assert_gathered(n, T, rows, f"counter {c:#x}")
        raw = ds.np()
        assert int(raw[0:8].view(np.uint64)[0]) == seed and raw[8:16].view(np.uint32).tolist() == [(c + 1) & 0xFFFFFFFF, 0] and ds.intact()


def test_uniform_draw_index_at_the_largest_replay():
    n = 2 ** 31 - 1
    lib = L.lib()
    for c in (0, 7, 0xFFFFFFFF):
        want = mp.draw_indices(77, c, 40, n)
        assert [lib.ivosw_replay_draw_index(77, c, b, n) for b in range(40)] == want.tolist()
        assert want.max() > 2 ** 30
    assert lib.ivosw_replay_draw_index(77, 0, 0, 0) == 0


# ---------------------------------------------------------------- e. the draw + gather inside the encoder launch
@pytest.mark.parametrize("n", [1, 3, 500])
@pytest.mark.parametrize("B,T", [(5, 9), (129, 25)])
def test_folded_draw_equals_the_draw_kernel(dev, B, T, n):
    """ivosw_dqn_step_drawn from counters 0xFFFFFFFF and 0 (captured: 8 kernel nodes say the folded chain ran, not the three calls)."""
    lib = L.lib()
    seed = 0xFEED_F00D
    NP = L.BRAIN_NPARAMS
    pol = torch.from_numpy(synth.brain_flat(synth.brain_state_dict(0))).to(dev)
    tgt = torch.from_numpy(synth.brain_flat(synth.brain_state_dict(1))).to(dev)
    grads, m, v = (torch.zeros(NP, device=dev) for _ in range(3))
    adam = torch.zeros(lib.ivosw_adam_state_bytes(), dtype=torch.uint8, device=dev)
    loss = Guarded(dev, 1, torch.float32)
    nbytes = lib.ivosw_dqn_ws_bytes(B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ds, ds_ref = draw_state(dev, seed, 0xFFFFFFFF), draw_state(dev, seed, 0xFFFFFFFF)
    out = Batch(dev, B, T)
    cols = columns(dev, n, T)
    torch.cuda.synchronize(dev)
    with L.Graph.capture(dev) as g:
        L.check(lib.ivosw_dqn_step_drawn(L.dptr(pol), L.dptr(tgt), *col_args(cols), L.dptr(ds.t), n, B, T, 0.95, L.dptr(out.idx.t),
                                         L.dptr(out.state.t), L.dptr(out.new_state.t), L.dptr(out.action.t), L.dptr(out.rstep.t),
                                         L.dptr(out.rdone.t), L.dptr(grads), L.dptr(loss.t), L.dptr(ws), nbytes, L.dptr(m), L.dptr(v), L.dptr(adam),
                                         5e-6, 0.9, 0.999, 1e-8, 5e-4, 1.0, 1.0, L.stream_ptr(dev)), "dqn_step_drawn")
    assert g.kernel_nodes == 8, g.kernel_nodes
    for c in (0xFFFFFFFF, 0):
        g.launch()
        torch.cuda.synchronize(dev)
        ref = uniform_draw(dev, n, B, T, ds_ref)
        rows = out.idx.np()
        np.testing.assert_array_equal(rows, mp.draw_indices(seed, c, B, n), err_msg=f"counter {c:#x}")
        for a, b, name in ((out.idx, ref.idx, "idx"), (out.state, ref.state, "state"), (out.new_state, ref.new_state, "new_state"),
                           (out.action, ref.action, "action"), (out.rstep, ref.rstep, "reward_step"), (out.rdone, ref.rdone, "reward_done")):
            assert torch.equal(a.t, b.t), (c, name)
        out.assert_gathered(n, T, rows, f"folded, counter {c:#x}")
        assert torch.equal(ds.t, ds_ref.t) and ds.intact() and loss.intact()
        assert ds.np()[8:16].view(np.uint32).tolist() == [(c + 1) & 0xFFFFFFFF, 0]
    assert np.isfinite(loss.np()).all()
