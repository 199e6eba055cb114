"""CPU: the J/F edge inputs of oracle/jf_cases.py.  Three jobs:
  1. every builder provably puts object pixels where it is named for (borders, the segment-seam columns, ids >= 128, 32 objects,
     4096 per wave, no empty bitmap word, the end of the buffer);
  2. the oracle (oracle/jf_oracle.py: numpy shifts + scipy dilation) equals a per-pixel, pair-by-pair restatement of the definition
     on the small border, tail and radius cases - it does not vouch for itself at the edges;
  3. the randomised inputs of tests/test_gpu_metrics.py hit none of these places (the gap these cases close)."""
import numpy as np
import pytest

from ivos_w_amd import synth
from oracle import jf_cases as jc
from oracle import jf_oracle as jo


# ---------------------------------------------------------------------------------------------- 1. the builders hit their targets
def _both_maps(case, probe, *a):
    return probe(case.gt, *a), probe(case.pred, *a)


@pytest.mark.parametrize("H,W,r", jc.BORDER_SHAPES)
def test_border_cases_touch_every_border(H, W, r):
    c = jc.border_case(H, W, r)
    assert c.gt.shape[1:] == (H, W) and c.gt.dtype == np.uint8 and c.pred.dtype == np.uint8
    for b in _both_maps(c, jc.border_pixels):
        assert min(b.values()) > 0, b
    N = c.gt.shape[0]
    assert (c.gt[: N // 2] == c.pred[N // 2:]).all() and (c.pred[: N // 2] == c.gt[N // 2:]).all()      # swapped copies
    per_frame_g, per_frame_p = c.gt.reshape(N, -1).sum(1), c.pred.reshape(N, -1).sum(1)
    assert ((per_frame_g > 0) & (per_frame_p == 0)).any() and ((per_frame_g == 0) & (per_frame_p > 0)).any()   # one map only
    assert (per_frame_g == H * W).any() and (per_frame_p == H * W).any()                                  # the full frame
    if H > 1 and W > 1:        # the corner pixel alone, the last row alone, the last column alone (each in both maps)
        for a in (c.gt, c.pred):
            assert any(f.sum() == 1 and f[-1, -1] for f in a)
            assert any(f.sum() == W and f[-1].all() for f in a)
            assert any(f.sum() == H and f[:, -1].all() for f in a)


def test_border_shapes_cover_the_grid():
    hs, ws = [s[0] for s in jc.BORDER_SHAPES], [s[1] for s in jc.BORDER_SHAPES]
    assert all(hs.count(h) == 3 for h in jc.BORDER_H) and all(ws.count(w) == 3 for w in jc.BORDER_W)
    shapes = {s[:2] for s in jc.BORDER_SHAPES}
    assert (1, 1) in shapes and any(h == 1 and w > 1 for h, w in shapes) and any(h > 1 and w == 1 for h, w in shapes)


@pytest.mark.parametrize("H,W", jc.SEAM_SHAPES)
def test_seam_cases_put_edges_on_the_seam(H, W):
    c = jc.seam_case(H, W)
    for a in (c.gt, c.pred):
        m = a == 1
        for col in jc.seam_columns(W):
            if col >= W:
                continue
            # a vertical edge exactly left of `col`, in both polarities, somewhere in this map
            left, here = m[:, :, col - 1], m[:, :, col]
            assert (left & ~here).any() and (~left & here).any(), col
        for s in (1023, 1024) + ((2047, 2048) if W == 2049 else ()):
            assert jc.column_pixels(a, s) > 0
            one = [f for f in m if f[:, s].all() and f.sum() == H]                 # the one-pixel column exactly there
            assert len(one) >= 1, s
        # the object spans the border between lanes 62 and 63 (columns 1007 | 1008): lane 62 must see lane 63's first pixel
        assert (m[:, :, 1007] & m[:, :, 1008]).any()
        # the south-east neighbour across the seam differs from the pixel: a diagonal edge passes 1023 -> 1024
        assert (m[:, :-1, 1023] != m[:, 1:, 1024]).any() and ((m[:, :-1, 1023] == m[:, :-1, 1024]) & (m[:, :-1, 1023] != m[:, 1:, 1024])).any()


@pytest.mark.parametrize("N,H,W", jc.TAIL_SHAPES)
def test_tail_cases_reach_the_end_of_the_buffer(N, H, W):
    c = jc.tail_case(N, H, W)
    assert jc.slow_path_loads(N, H, W) > 0
    flat = c.gt.reshape(-1)
    if N * H > 1:
        # the bytes right behind the end of an object-free row end belong to the object: an unmasked 16-byte load would count them
        ends = [((n * H + y) + 1) * W for n in range(N) for y in range(0, H, 2) if (n * H + y + 1) < N * H and not (n > 0 and y == 0)]
        assert ends and all(flat[e] == 1 for e in ends)
    if N > 1:
        assert flat[(N - 1) * H * W] == 1            # first pixel of the next frame right behind the last row of the one before


def test_id_cases_use_the_whole_byte_range():
    c = jc.iid_bytes_case()
    assert len(np.unique(c.gt)) == 256 and len(np.unique(c.pred)) == 256
    u = jc.unique_ids_case()
    assert u.nb_objects is None
    assert tuple(jo._object_ids(u.gt.astype(np.int64), None)) == jc.UNIQUE_IDS and (u.gt == 255).any() and (u.pred == 255).any()
    assert max(jc.UNIQUE_IDS) >= 128 and all((u.pred == v).any() for v in jc.UNIQUE_IDS)
    m = jc.many_objects_case()
    assert m.nb_objects == 32 and all((m.gt == v).any() and (m.pred == v).any() for v in range(1, 33)) and (m.pred == 33).any()
    ids = list(jc.CABI_IDS)
    assert ids != sorted(ids) and len(set(ids)) == len(ids) and {0, 255, 127, 128} <= set(ids)


def test_dense_cases_fill_the_words_and_the_counters():
    for c, ids in ((jc.checkerboard_case(), [1]), (jc.coin_flip_case(), [1, 2])):
        assert jc.empty_word_share(c.gt, c.pred, ids[:1]) == 0.0
    for c in jc.full_wave_case():
        assert jc.max_per_wave(c.gt, c.pred, [1]) == (4096, 4096)
        assert c.gt.shape[1] % 16 == 0 and c.gt.shape[2] % 1024 == 0


@pytest.mark.parametrize("r", jc.RADII)
def test_radius_cases_sit_on_the_disks_rim(r):
    hw = jc.half_widths(r)
    d = jo.disk(r)
    assert [int(d[r + k].sum() - 1) // 2 for k in range(r + 1)] == hw                  # the oracle's disk has these half widths
    assert jc.RADIUS_W >= 100
    offs = set()
    for part in ("row", "col", "rim"):
        c = jc.radius_case(r, part)
        assert c.bound_th == r and c.gt.shape[2] == jc.RADIUS_W
        for g, p in zip(c.gt, c.pred):
            assert g.sum() == 1 and p.sum() == 1
            (gy, gx), (py, px) = np.argwhere(g)[0], np.argwhere(p)[0]
            offs.add((int(py - gy), int(px - gx)))
            assert gx // 32 != (px - 1) // 32 or r < 3 or part != "row"                 # the row pairs lie in different bitmap words
    for k in range(2):
        assert (0, r + k) in offs and (r + k, 0) in offs                               # distance exactly r and exactly r + 1
        for dy in {x for x in (1, r // 2, r - 1) if 0 < x <= r}:
            assert (dy, hw[dy] + k) in offs and hw[dy] ** 2 + dy ** 2 <= r * r < (hw[dy] + 1) ** 2 + dy ** 2
    # boundary pixels within r of every border, in both maps, and in the first and the last bitmap word
    c = jc.radius_case(r, "frame")
    H, W = c.gt.shape[1:]
    for a in (c.gt, c.pred):
        b = np.stack([jo.seg2bmap(f == 1) for f in a]).any(0)
        ys, xs = np.nonzero(b)
        assert ys.min() <= r and ys.max() >= H - 1 - r and xs.min() <= r and xs.max() >= W - 1 - r
        assert b[:, :32].any() and b[:, 128:].any()


# ---------------------------------------------------------------------------------------------- 2. the oracle against the definition
def _assert_oracle_is_the_definition(c, frames=None):
    ids = [1]
    r = int(jo.bound_pixels(c.gt.shape[1:], c.bound_th))
    got = jc.counts(c.gt, c.pred, ids, r)
    for n in (range(c.gt.shape[0]) if frames is None else frames):
        assert got[n, 0].tolist() == jc.brute_counts(c.gt[n] == 1, c.pred[n] == 1, r), n
        f = jo.f_measure(c.gt[n] == 1, c.pred[n] == 1, bound_th=c.bound_th)
        assert f == jo.pr_to_f(*got[n, 0, 2:].tolist())


@pytest.mark.parametrize("H,W,r", [s for s in jc.BORDER_SHAPES if s[0] * s[1] <= 17 * 17])
def test_oracle_equals_brute_force_on_small_border_cases(H, W, r):
    _assert_oracle_is_the_definition(jc.border_case(H, W, r))


@pytest.mark.parametrize("N,H,W", [s for s in jc.TAIL_SHAPES if s[2] < 64])
def test_oracle_equals_brute_force_on_tail_cases(N, H, W):
    _assert_oracle_is_the_definition(jc.tail_case(N, H, W))


@pytest.mark.parametrize("r,part", [(0, "row"), (1, "row"), (1, "rim"), (7, "rim"), (8, "col"), (9, "rim"), (32, "row")])
def test_oracle_equals_brute_force_on_rim_pairs(r, part):
    _assert_oracle_is_the_definition(jc.radius_case(r, part))


def test_j_and_f_from_counts_are_the_oracles():
    """jc.j_and_f (used where the dilation is dear) returns what jo.batched_jaccard / jo.batched_f_measure return."""
    for c, ids in ((jc.border_case(5, 17, 1), [1]), (jc.many_objects_case(), list(range(1, 33))), (jc.radius_case(7, "frame"), [1])):
        r = int(jo.bound_pixels(c.gt.shape[1:], c.bound_th))
        j, f = jc.j_and_f(jc.counts(c.gt, c.pred, ids, r))
        np.testing.assert_array_equal(j, jo.batched_jaccard(c.gt, c.pred, False, c.nb_objects))
        np.testing.assert_array_equal(f, jo.batched_f_measure(c.gt, c.pred, False, c.nb_objects, c.bound_th))


# ---------------------------------------------------------------------------------------------- 3. what the older inputs never reach
def _old_inputs():
    from tests import test_gpu_metrics as old
    mark = [m for m in old.test_counts_and_metrics_match_oracle.pytestmark if m.name == "parametrize"][0]
    for (N, H, W, O, bth) in mark.args[1]:
        gt, pr = synth.label_maps(N, H, W, O, seed=N * 1000 + W, void=(O > 1))
        noise = np.random.RandomState(5).rand(N, H, W) < 0.002
        yield (N, H, W, O, bth), gt, pr, np.where(noise, (pr + 1) % (O + 1), pr).astype(np.uint8)


def test_randomised_inputs_of_the_older_test_miss_these_places():
    n_cases = 0
    for (N, H, W, O, bth), gt, clean, pr in _old_inputs():
        n_cases += 1
        assert sum(jc.border_pixels(gt).values()) == 0, (H, W)                     # gt: no object pixel on any border
        assert sum(jc.border_pixels(clean).values()) == 0                           # pred: none either before the noise ...
        bp = jc.border_pixels(pr)                                                   # ... and a few stray noise pixels after it
        assert bp["top"] + bp["bottom"] + bp["left"] + bp["right"] <= 0.004 * 2 * N * (H + W) + 2 and bp["corner"] == 0
        if W > 1024:
            for a in (gt, pr):
                assert jc.column_pixels(a, 1023) == 0 and jc.column_pixels(a, 1024) == 0              # the seam's east neighbour is never set
                assert jc.column_pixels(a, 1008) == 0          # nor the first pixel of lane 63, which lane 62 reads as ITS east neighbour
        assert max(gt[gt < 255].max(), pr.max()) <= 4                               # ids 1..4: the high bit of a label byte is never set
        if N * H * W <= 2_000_000:
            assert max(jc.max_per_wave(gt, pr, range(1, O + 1))) < 4096
    assert n_cases == 11
