"""TEST INFRASTRUCTURE (never imported by the product path): exact references and named cases for the replay kernels of
csrc/dqn.hip - the prioritized draw (per_draw_gather_kernel), the sum-tree build and update (per_leaves_kernel /
per_level_kernel / per_update_kernel) and the uniform draw - that do NOT share the kernels' arithmetic.  The host mirrors in
models/momory_pool.py (per_draw_rows, per_update_host) restate the kernels step by step in float32; the models here state what
the steps must add up to.  tests/test_oracle_per_cases.py holds both against each other without a GPU.

The exact model of the prioritized draw
---------------------------------------
The kernel gives slot b of a B-slot draw the point x = (total / B) * ((float)b + u), u = k * 2^-24 with k the top 24 bits of
draw_mix(seed, counter, b), and walks from the root: left when x < left child, else x -= left child and right.  Take a tree
whose leaves are non-negative INTEGERS with total < 2^24 and total / B a power of two (``assert_exact_draw_case``).  Then
  * every node is an integer below 2^24: every float32(left + right) of the build is exact, the root IS the total;
  * step = total / B is exact, and a product with a power of two is exact, so x = step * float32(b + u): the one rounding of
    the whole draw is the plain IEEE addition b + u (u itself is exact: k < 2^24);
  * at a node the walk holds 0 <= x <= total < 2^24, hence ulp(x) <= 1 and the integer `left` is a multiple of ulp(x); when
    the walk goes right, left <= x, so x - left is a non-negative multiple of ulp(x) no larger than x: representable, exact.
So the walk is the exact walk: below a node with sum S it arrives with 0 <= x < S (x == total at the root excepted), goes left
iff x < left, and ends at the leaf i with c[i-1] <= x < c[i], c = the running sum of the leaves - a leaf with c[i] > c[i-1],
never a zero one, never padding.  That is the number of running sums <= x:

    row = searchsorted(cumsum(leaves, float64), x, side="right")

and when float32(b + u) rounded up to B (slot B - 1, u within half an ulp of 1) x == total, no running sum exceeds it, the
walk goes right at every level to leaf P - 1, and the kernel's min(., n - 1) gives row n - 1 - the value searchsorted's n is
clamped to.  (With a zero last leaf that row has priority 0 and an infinite weight: per_update cannot write a zero leaf, eps
> 0, so the generators keep the last row non-zero and nothing here tests it.)

Weights: w_b = (leaf_b * n / total) ** -beta / max_b(.), beta = beta0 + (1 - beta0) * min(c, N) / N (beta0 at N = 0), in
float64 from the float32 leaves, and the same expression evaluated in float32 numpy - whose distance from float64 is the
yardstick for the kernel's (tests/test_gpu_replay_edges.py).

Update: given the new leaf values, the last slot of a repeated row wins, rows outside [0, n) are skipped, every internal
node is float32(left + right) of its children (the tree is a pure function of its leaves, so the model rebuilds all of
them), and max_priority = max(old, max over ALL slots of float32(td + eps)), skipped ones included (include/ivosw.h).
"""
import functools

import numpy as np

_M64 = (1 << 64) - 1
INT64_MIN = -(1 << 63)


# ------------------------------------------------------------------------------------------------ tree helpers
def tree_leaves(n):
    """P: the next power of two >= max(n, 2)."""
    P = 2
    while P < n:
        P *= 2
    return P


def rebuild(leaves, n=None):
    """float32 [2P] tree of the given leaves (zero padding, slot 0 = 0), every internal node float32(left + right)."""
    leaves = np.asarray(leaves, np.float32)
    n = leaves.shape[0] if n is None else n
    P = tree_leaves(n)
    t = np.zeros(2 * P, np.float32)
    t[P:P + n] = leaves[:n]
    lo = P // 2
    while lo >= 1:
        pair = t[2 * lo:4 * lo].reshape(lo, 2)
        t[lo:2 * lo] = pair[:, 0] + pair[:, 1]
        lo //= 2
    return t


# ------------------------------------------------------------------------------------------------ the draw
def mix(seed, counter, slots):
    """draw_mix(seed, counter, slot) for an array of slots: uint64 numpy arithmetic (wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        s = np.asarray(slots, np.uint64)
        z = (np.uint64(seed & _M64) + np.uint64((0x9E3779B97F4A7C15 * ((counter & 0xFFFFFFFF) + 1)) & _M64)
             + np.uint64(0xD1B54A32D192ED03) * (s + np.uint64(1)))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw_points(total, seed, counter, B):
    """float32 [B]: step * float32(b + u), step = float32(total / B) - exact when total / B is a power of two."""
    u = (mix(seed, counter, np.arange(B)) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    bu = np.arange(B, dtype=np.float32) + u                    # the one rounded operation
    return (np.float32(total) / np.float32(B)) * bu


def assert_exact_draw_case(leaves, B):
    """The conditions under which ``exact_draw_rows`` IS the kernel's answer."""
    lv = np.asarray(leaves)
    assert lv.ndim == 1 and lv.shape[0] >= 1
    assert np.all(lv >= 0) and np.all(lv == np.floor(lv)), "integer leaves"
    total = int(np.asarray(lv, np.float64).sum())
    assert 0 < total < 2 ** 24, total
    q = total / B
    m, _ = np.frexp(q)
    assert m == 0.5 and q * B == total, f"total / B = {total} / {B} is not a power of two"
    assert lv[-1] > 0, "the last row must be drawable (x == total lands on it)"
    return total


def exact_draw_rows(leaves, seed, counter, B):
    """Rows of draw `counter` on an integer-leaf tree (see the module docstring) -> int64 [B]."""
    total = assert_exact_draw_case(leaves, B)
    n = len(leaves)
    x = draw_points(total, seed, counter, B).astype(np.float64)
    c = np.cumsum(np.asarray(leaves, np.float64), dtype=np.float64)
    return np.minimum(np.searchsorted(c, x, side="right"), n - 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ weights
def beta64(beta0, beta_steps, counter):
    b0 = np.float64(np.float32(beta0))
    if beta_steps == 0:
        return b0
    return b0 + (1.0 - b0) * (min(int(counter) & 0xFFFFFFFF, int(beta_steps)) / np.float64(beta_steps))


def weights64(leaves, rows, beta0, beta_steps, counter):
    """float64 [B]: (leaf * n / total) ** -beta over its maximum; leaves = the float32 leaves, total their float64 sum."""
    lv = np.asarray(leaves, np.float32).astype(np.float64)
    n = lv.shape[0]
    w = (lv[rows] * n / lv.sum()) ** -beta64(beta0, beta_steps, counter)
    return w / w.max()


def weights32(leaves, root, rows, beta0, beta_steps, counter):
    """The same expression in float32 numpy, every operation rounded to float32 (root = the tree's float32 total)."""
    f = np.float32
    lv = np.asarray(leaves, np.float32)
    n = lv.shape[0]
    b0 = f(beta0)
    beta = b0 if beta_steps == 0 else f(b0 + f(f(1) - b0) * f(f(min(int(counter) & 0xFFFFFFFF, int(beta_steps))) / f(beta_steps)))
    w = np.power(lv[rows] * f(n) / f(root), -beta, dtype=np.float32)
    return w / w.max()


# ------------------------------------------------------------------------------------------------ update
def update_winners(idx, n):
    """{row: slot} - the last slot of a repeated row wins, rows outside [0, n) are skipped."""
    win = {}
    for b, r in enumerate(np.asarray(idx, np.int64).tolist()):
        if 0 <= r < n:
            win[r] = b
    return win


def update_model(tree, n, idx, new_leaf_of_slot):
    """The tree after an update that sets row idx[b]'s leaf to new_leaf_of_slot[b] (float32 [B]) -> float32 [2P].
    `tree` must be consistent (== rebuild of its own leaves): the update keeps that property."""
    t = np.asarray(tree, np.float32)
    P = t.shape[0] // 2
    assert P == tree_leaves(n) and np.array_equal(rebuild(t[P:], P).view(np.uint32), t.view(np.uint32)), "inconsistent tree"
    lv = t[P:].copy()
    for r, b in update_winners(idx, n).items():
        lv[r] = np.float32(new_leaf_of_slot[b])
    return rebuild(lv, P)


def update_max_priority(max_priority, td, eps):
    """float32 max(old, max over every slot of float32(td + eps))."""
    p = np.asarray(td, np.float32) + np.float32(eps)
    return np.float32(max(np.float32(max_priority), p.max()))


def update_leaf64(td, eps, alpha):
    """float64 [B]: float32(td + eps) ** alpha, the value a winning slot's leaf is held to (2 ulp)."""
    p = (np.asarray(td, np.float32) + np.float32(eps)).astype(np.float64)
    return p ** np.float64(np.float32(alpha))


# ------------------------------------------------------------------------------------------------ case generators
def int_leaves(n, B, seed=0):
    """Integer leaves 0..7 (about a third of them 0) whose last row is non-zero and whose total is B * 2^k: float64 [n]."""
    rs = np.random.RandomState(1000003 * seed + 31 * n + B)
    lv = rs.randint(0, 8, n).astype(np.float64)
    lv[rs.rand(n) < 0.33] = 0
    if n > 2:
        lv[0] = 0                       # x == 0 must walk past a zero first leaf
    rest = int(lv[:-1].sum())
    total = B
    while total <= rest:
        total *= 2
    lv[-1] = total - rest
    assert_exact_draw_case(lv, B)
    assert n <= 2 or (lv[:-1] == 0).any()
    return lv


def boundary_leaves(seed, counter, front_zeros=0, B=1024):
    """Integer leaves, total 2^23, whose running sums ARE the points of draw `counter`: at step = 2^13 the slots b >= 512 have
    float32(b + u) on a 2^-14 grid, so x is a multiple of 1/2 and about half of them are integers; every such x becomes a running sum
    (x == left child at some level of the walk: `<` against `<=`), every fourth one is followed by a zero leaf, `front_zeros` zero
    leaves come first.  -> (float64 [n], the slots whose x is a running sum)."""
    total = 2 ** 23
    x = draw_points(total, seed, counter, B).astype(np.float64)
    on = np.flatnonzero((x == np.floor(x)) & (x > 0) & (x < total))
    cuts = np.unique(x[on])
    lv = []
    for k, d in enumerate(np.diff(np.concatenate([[0.0], cuts, [float(total)]]))):
        lv.append(d)
        if k % 4 == 3:
            lv.append(0.0)
    lv = np.array([0.0] * front_zeros + lv)
    if lv[-1] == 0:
        lv = lv[:-1]
    assert_exact_draw_case(lv, B)
    assert len(on) >= B // 8 and np.isin(x[on], np.cumsum(lv)).all()
    return lv, on


def beta_leaves(n=1000, B=64):
    """Integer leaves that are powers of two 2^0 .. 2^12 (the last one takes the remainder to a total of B * 2^14): the drawn leaves
    are a factor 2^12 apart, so a beta off by one step of 40 moves the smallest weight by 12 %.  float64 [n]."""
    rs = np.random.RandomState(3)
    lv = np.ldexp(1.0, rs.randint(0, 13, n)).astype(np.float64)
    lv[-1] += B * 2 ** 14 - lv.sum()
    assert_exact_draw_case(lv, B)
    return lv


def hot_pair_leaves(seed, counter, n=1000, slot=100, B=1024):
    """Integer leaves, total 2^23: a heavy last leaf with half of the mass (2^22) and a light leaf of 8 (2^-20 of the mass) laid under
    the point of `slot` in draw `counter`, so that BOTH are drawn and the weights span a ratio of 2^19; n - 3 fillers of about
    slot * 2^13 / (n - 3) in front of the light leaf, one behind it.  -> (float64 [n], the light leaf's row)."""
    total = 2 ** 23
    x = float(draw_points(total, seed, counter, B)[slot])
    front = int(np.floor(x)) - 3                       # the light leaf covers [front, front + 8), x inside
    k = n - 3
    fill = np.full(k, front // k, np.float64)
    fill[:front % k] += 1
    lv = np.concatenate([fill, [8.0, float(total // 2 - front - 8), float(total // 2)]])
    assert_exact_draw_case(lv, B)
    assert len(lv) == n and lv[:k].sum() == front and front <= x < front + 8 and lv[k + 1] > 0
    return lv, k


def hot_leaves(n, hot=None):
    """One leaf of 1.0 that carries all but 1e-30 of the mass: float32 [n]."""
    hot = n // 3 if hot is None else hot
    lv = np.full(n, 1e-30 / max(n - 1, 1), np.float32)
    lv[hot] = 1.0
    return lv


def wide_leaves(n, seed=0):
    """Leaves log-uniform over 1e-20 .. 1e20, both ends present: float32 [n]."""
    rs = np.random.RandomState(77 + seed)
    lv = (10.0 ** rs.uniform(-20, 20, n)).astype(np.float32)
    if n >= 2:
        lv[0], lv[-1] = 1e-20, 1e20
    return lv


def update_patterns(n, B_max=1024):
    """{name: int64 rows} - the index patterns of per_update_kernel's list of touched nodes that fit a tree of n rows."""
    rs = np.random.RandomState(5 + n)
    pats = {"one_slot": np.array([n // 2]), "one_row_everywhere": np.full(B_max, n // 2), "last_row": np.array([n - 1]),
            "first_and_last": np.array([0, n - 1]), "first_and_last_repeated": np.array([0, n - 1] * 33 + [0]),
            "out_of_range": np.array([-1, n, 2 ** 40, INT64_MIN]),
            "out_of_range_between": np.array([n, 0, -1, n - 1, 2 ** 40, n // 2, INT64_MIN]),
            "random_with_repeats": rs.randint(0, n, 257)}
    for s in (0, 1, 1023):
        m = min(B_max, n - s)
        if m < 2:
            continue
        run = np.arange(s, s + m)
        pats[f"run{s}_ascending"] = run
        pats[f"run{s}_descending"] = run[::-1].copy()
        pats[f"run{s}_shuffled"] = rs.permutation(run)
    return {k: np.asarray(v, np.int64) for k, v in pats.items()}


@functools.lru_cache(maxsize=None)
def rounded_up_slot(seed=0x5EED, B=1024, limit=1 << 20):
    """(seed, counter): the first counter at which slot B - 1 of a B-slot draw has float32((B - 1) + u) == B.  Searched through the
    host mirror's own _draw_mix (one draw in 2^15 at B = 1024: u >= 1 - 2^-15)."""
    from ivos_w_amd.models.momory_pool import _draw_mix
    f = np.float32
    for c in range(limit):
        u = f(f(_draw_mix(seed, c, B - 1) >> 40) * f(2.0 ** -24))
        if f(f(B - 1) + u) == f(B):
            return seed, c
    raise AssertionError("no rounded-up slot found")
