"""tests/dqn_ref.py on the CPU: its float64 restatements, composed in the step's order, ARE oracle.brain_oracle.dqn_loss_and_grads and
oracle.brain_oracle.brain_forward in float64, and its fixtures have the properties the GPU tests (tests/test_gpu_dqn_kernels.py,
tests/test_gpu_dqn_fwd_kernels.py) lean on."""
import numpy as np
import pytest

from oracle import brain_oracle as O
from tests import dqn_ref as R

SHAPES = {"encoder_fc1.weight": (128, 2), "encoder_fc1.bias": (128,), "encoder_fc2.weight": (128, 128), "encoder_fc2.bias": (128,),
          "lstm_cell.weight_ih": (512, 128), "lstm_cell.weight_hh": (512, 128), "decoder_fc1.weight": (128, 256), "decoder_fc1.bias": (128,),
          "decoder_fc2.weight": (1, 128), "decoder_fc2.bias": (1,)}
EXACT_LIMIT = 2.0 ** 24


def _params(rng):
    return {k: (rng.uniform(-1, 1, s) / np.sqrt(s[-1] if len(s) > 1 else 128)).astype(np.float32) for k, s in SHAPES.items()}


def _batch(rng, B, T):
    col = lambda: rng.uniform(0, 1, (B, 1, T))
    action = rng.integers(0, T, (B, 1))
    action[0, 0], action[-1, 0] = 0, T - 1
    return {"old_state_iou": col(), "new_state_iou": col(), "annotated_frames": (col() > 0.7).astype(np.float64),
            "next_annotated_frames": (col() > 0.6).astype(np.float64), "action": action, "reward_step": rng.uniform(-1, 1, (B, 1)),
            "reward_done": rng.uniform(-1, 1, (B, 1))}


@pytest.mark.parametrize("B,T", [(5, 9), (3, 4)])
def test_the_restatements_composed_are_the_oracle_in_float64(B, T):
    """head -> bptt -> tail_grads on the oracle's own forward reproduce loss and all ten gradient tensors to 1e-12 of each tensor's scale."""
    rng = np.random.default_rng([1, B, T])
    P, Pt, batch, gamma = _params(rng), _params(rng), _batch(rng, B, T), 0.99
    f = np.float64
    loss_o, G_o = O.dqn_loss_and_grads(P, Pt, batch, gamma, dtype=f)
    state, new_state = O.build_states(batch, f)
    action = np.asarray(batch["action"]).reshape(-1)
    f32 = lambda k: np.asarray(batch[k]).reshape(-1).astype(np.float32)
    q_np, q_nt = O.brain_forward(P, new_state, f), O.brain_forward(Pt, new_state, f)
    q_s, c = O.brain_forward(P, state, f, keep=True)
    hs = np.concatenate([c["hs"][0], c["hs"][1]], 2)
    hd = R.head(P["decoder_fc1.weight"], P["decoder_fc2.weight"][0], q_np, q_nt, q_s, action, f32("reward_step"), f32("reward_done"), gamma,
                R.LOSS_MSE, 1.0, c["d1"], hs, dtype=f)
    dG = R.bptt(P["lstm_cell.weight_hh"], c["gates"], c["cs"], hd["dhc"], action, f)
    assert not dG[~R.live_frames(action, B, T)].any(), "frames past the loss frame carry no gradient"
    hprev = np.zeros_like(c["hs"])
    hprev[0, :, 1:], hprev[1, :, :-1] = c["hs"][0, :, :-1], c["hs"][1, :, 1:]
    rows = B * T
    _, _, G = R.tail_grads(dG.reshape(2, rows, 512), hprev.reshape(2 * rows, 128), c["e"].reshape(rows, 128), c["a1"].reshape(rows, 128),
                           hd["dd1c"], hd["hcc"], hd["w4term"], state.reshape(rows, 2), P["lstm_cell.weight_ih"], P["encoder_fc2.weight"], f)
    G["decoder_fc2.bias"] = hd["db4"].reshape(1)
    assert abs(hd["loss"] - loss_o) <= 1e-12 * abs(loss_o)
    assert sorted(G) == sorted(G_o) and set(R.TAIL_KEYS) | {"decoder_fc2.bias"} == set(G_o)
    for k, want in G_o.items():
        assert G[k].shape == want.shape == SHAPES[k], k
        assert np.abs(G[k] - want).max() <= 1e-12 * np.abs(want).max(), k


def test_the_arena_table_is_the_state_dict_layout():
    off = 0
    for (k, o, s), (k2, s2) in zip(R.ARENA, SHAPES.items()):
        assert (k, s) == (k2, s2) and o == off
        off += int(np.prod(s))
    assert off == R.NPARAMS


def test_slab_rows_cut_as_the_kernels_do():
    assert R.slab_rows(97, 7, 16) == [(0, 16), (16, 32), (32, 48), (48, 64), (64, 80), (80, 96), (96, 97)]
    assert R.slab_rows(97, 3, 16) == [(0, 48), (48, 96), (96, 97)]
    assert R.slab_rows(33, 3, 16) == [(0, 16), (16, 32), (32, 33)]
    assert R.slab_rows(1, 8, 8) == [(0, 1)] + [(1, 1)] * 7                      # empty splits
    assert R.slab_rows(17, 7, 16)[2:] == [(17, 17)] * 5                         # empty trailing slabs
    assert R.slab_rows(520, 8, 8) == [(72 * z, min(520, 72 * z + 72)) for z in range(8)]
    A, B = R.ints(np.random.default_rng(0), (97, 64)), R.ints(np.random.default_rng(1), (97, 128))
    assert np.array_equal(R.wgrad_slabs(A, None, B, 7).sum(0), R.wgrad(A, None, B))


def _is_integer(t):
    return bool((np.asarray(t, np.float64) == np.round(np.asarray(t, np.float64))).all())


def test_exact_wgrad_fixtures_have_integer_partial_sums_below_2_24():
    for M, N, _ in R.WG_SHAPES:
        for K, nslab in [(k, 1) for k in R.WG_K1] + list(R.WG_SPLITS) + [(k, 1) for k, _ in R.WG_AUTO]:
            for has2 in (False, True):
                A, A2, B = R.wgrad_fixture(M, N, K, has2, True)
                assert all(_is_integer(t) for t in (A, B) + ((A2,) if has2 else ()))
                assert R.wgrad_mag(A, A2, B, 1).max() < EXACT_LIMIT            # one slab bounds every split of it


def test_exact_dgrad_csum_and_group_fixtures_have_integer_partial_sums_below_2_24():
    for rows in R.DG_ROWS:
        dG, dG2, wih, w2, a1 = R.dgrad_fixture(rows, True)
        assert all(_is_integer(t) for t in (dG, dG2, wih, w2, a1)) and R.has_every_mask_class(a1, integer=True)
        de = (np.abs(dG) + np.abs(dG2)).astype(np.float64) @ np.abs(wih)
        assert de.max() <= 4096 and (de @ np.abs(w2)).max() <= 2 ** 20
    for M in R.CS_M:
        A, x = R.csum_fixture(M, 128, True, True)
        assert _is_integer(A) and _is_integer(x)
        assert (np.abs(A).astype(np.float64).T @ np.maximum(np.abs(x), 1)).max() < EXACT_LIMIT
    for B, T in R.GROUP_BT:
        fx = R.group_fixture(B, T)
        assert all(_is_integer(t) for t in fx.values()) and R.has_every_mask_class(fx["a1"], integer=True)
        assert R.tail_mags(**fx) < EXACT_LIMIT, (B, T)


def test_dense_fixtures_hold_every_mask_class():
    for rows in R.DG_ROWS:
        a1 = R.dgrad_fixture(rows, False)[4]
        assert all(R.has_every_mask_class(r) for r in a1), rows         # every row: a tail tile of one row still sees them all
    for B, T in ((1, 1), (2, 65), (257, 63)):
        fx = R.head_fixture(B, T)
        a = np.clip(fx["action"], 0, T - 1)
        assert R.has_every_mask_class(fx["d1"][np.arange(B), a]) and R.has_every_mask_class(fx["hs"][np.arange(B), a])
    t = R.with_mask_classes(np.ones((3, 128), np.float32))
    assert R.has_every_mask_class(t) and not R.has_every_mask_class(np.ones((3, 128), np.float32))


def test_head_fixture_has_its_ties_thresholds_and_actions():
    cases = R.head_cases()
    assert {c[0] for c in cases} == set(R.HEAD_B) and {c[1] for c in cases} == set(R.HEAD_T)
    assert {(c[2], c[3]) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for B, T in ((3, 65), (257, 64), (2, 1)):
        fx = R.head_fixture(B, T)
        q = fx["q_np"]
        assert q[0, 0] == q[0, T - 1] == q[0].max() and R.first_argmax(q)[0] == 0            # tie at the first and last frame
        assert (q[1] == q[1, 0]).all() and R.first_argmax(q)[1] == 0                           # all equal
        if B > 2 and T > 1:
            assert q[2, 14 % T] == q[2, T - 1] == q[2].max() and R.first_argmax(q)[2] == min(14 % T, T - 1)
        assert {0, T - 1} <= set(fx["action"].tolist())
        for dt in (np.float32, np.float64):
            h = R.head(fx["W3"], fx["w4"], q, fx["q_nt"], fx["q_s"], fx["action"], fx["r_step"], fx["r_done"], R.HEAD_GAMMA, R.LOSS_HUBER,
                       R.HEAD_DELTA, fx["d1"], fx["hs"], fx["weights"], dt)
            assert (h["e2"][:min(B, 3)] == R.HEAD_DELTA).all()
            assert np.array_equal(h["e1"][:min(B, 3)], np.array([0.125, 0.5, -1.0], dt)[:min(B, 3)])      # below, at and above delta
    # on this grid the fp32 restatement's e1, e2 do not depend on contraction: qn * gamma and r * 0.1f are exact in fp32
    fx = R.head_fixture(257, 65)
    qn = fx["q_nt"][np.arange(257), R.first_argmax(fx["q_np"])]
    assert np.array_equal((qn * np.float32(R.HEAD_GAMMA)).astype(np.float64), qn.astype(np.float64) * R.HEAD_GAMMA)
    for r in (fx["r_step"], fx["r_done"]):
        assert np.array_equal((r * np.float32(0.1)).astype(np.float64), r.astype(np.float64) * np.float64(np.float32(0.1))) and len(set(r.tolist())) > 4


def test_head_huber_equals_mse_inside_delta_and_clamps_outside():
    fx = R.head_fixture(4, 3)
    args = (fx["W3"], fx["w4"], fx["q_np"], fx["q_nt"], fx["q_s"], fx["action"], fx["r_step"], fx["r_done"], R.HEAD_GAMMA)
    big = R.head(*args, R.LOSS_HUBER, 1e6, fx["d1"], fx["hs"])
    mse = R.head(*args, R.LOSS_MSE, 1.0, fx["d1"], fx["hs"])
    assert np.allclose(2 * big["loss"], mse["loss"], rtol=1e-14) and np.allclose(2 * big["dq_own"], mse["dq_own"], rtol=1e-14)
    hub = R.head(*args, R.LOSS_HUBER, R.HEAD_DELTA, fx["d1"], fx["hs"])
    assert hub["dq_own"][2] == (np.clip(-1.0, -0.5, 0.5) + 0.5) / 4 == 0.0 and hub["dq_own"][0] == (0.125 + 0.5) / 4


def test_lstm_fixture_covers_first_last_and_middle_loss_frames():
    for N in (1, 3, 130):
        for T in R.LSTM_T:
            fx = R.lstm_fixture(N, T)
            a = fx["action"]
            assert a.min() == 0 and (N < 2 or a.max() == T - 1) and (N < 3 or T < 3 or (T // 2) in a)
            live = R.live_frames(a, N, T)
            assert live[0].sum(1).tolist() == (a + 1).tolist() and live[1].sum(1).tolist() == (T - a).tolist()
    fx = R.lstm_fixture(130, 9)
    assert len({int(v) for v in fx["action"][:4]}) >= 3          # rows of one workgroup (forms 2 and 4) stop at different steps
    ref = R.bptt(**fx)
    assert not ref[~R.live_frames(fx["action"], 130, 9)].any() and np.abs(ref[R.live_frames(fx["action"], 130, 9)]).min(-1).max() > 0


# ---------------------------------------------------------------- the forward restatements and fixtures
def _close(got, want, what):
    assert got.shape == want.shape, what
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what


@pytest.mark.parametrize("N,T", [(5, 9), (3, 1), (2, 4)])
def test_the_forward_restatements_composed_are_the_oracle_in_float64(N, T):
    """enc -> lstm_fwd -> dec reproduce the oracle's q and every tensor it keeps to 1e-12 of each tensor's scale; hprev is hs of the frame
    the direction consumed before; lstm_fwd is lstm_step frame by frame."""
    rng = np.random.default_rng([2, N, T])
    P = _params(rng)
    x = rng.uniform(-1, 1, (N, T, 2))
    q_o, c = O.brain_forward(P, x, np.float64, keep=True)
    assert R.SHAPES == SHAPES
    a1, e, gx = R.enc(P, x.reshape(-1, 2))
    hs, gates, cs, hprev = R.lstm_fwd(P["lstm_cell.weight_hh"], gx.reshape(N, T, 512))
    d1, q = R.dec(P, hs.reshape(-1, 256))
    _close(a1.reshape(N, T, 128), c["a1"], "a1")
    _close(e.reshape(N, T, 128), c["e"], "e")
    _close(hs, np.concatenate([c["hs"][0], c["hs"][1]], 2), "hs")
    _close(gates, c["gates"], "gates")
    _close(cs, c["cs"], "cs")
    _close(d1.reshape(N, T, 128), c["d1"], "d1")
    _close(q.reshape(N, T), q_o, "q")
    want = np.zeros_like(c["hs"])                        # (the step's hprev of test_the_restatements_composed_are_the_oracle_in_float64)
    want[0, :, 1:], want[1, :, :-1] = hs[:, :-1, :128], hs[:, 1:, 128:]
    assert np.array_equal(hprev, want)
    for d, t in ((0, T - 1), (1, 0)):                    # the last step of either direction, from the chain's own state
        tp = R.prev_frame(d, t)
        cprev = cs[d, :, tp] if 0 <= tp < T else np.zeros((N, 128))
        g, cc, h = R.lstm_step(P["lstm_cell.weight_hh"], gx.reshape(N, T, 512)[:, t], hprev[d, :, t], cprev)
        assert np.array_equal(g, gates[d, :, t]) and np.array_equal(cc, cs[d, :, t]) and np.array_equal(h, hs[:, t, d * 128:(d + 1) * 128])
    assert np.array_equal(R.arena(P)[82432:82432 + 512 * 128].reshape(512, 128), P["lstm_cell.weight_hh"])


def test_forward_case_tables_reach_every_tile_edge():
    assert R.enc_cases(1) == [(1, 0), (1, 1)]
    assert R.enc_cases(48) == [(48, 0), (48, 48), (1, 0), (1, 48)]
    assert set(R.enc_cases(97)) == {(r0, k) for r0 in (97, 50, 1) for k in (0, 50, 97)}       # both thresholds inside the second tile
    assert R.ENC_ROWS == (1, 47, 48, 49, 97) and [r for r, _, _ in R.TWO_JOBS] == [49, 47]
    assert [R.product_form(N) for N in (3, 4, 130)] == [11, 20, 20]
    assert R.FWD_T == (1, 2, 3, 9) and R.FWD_N_SMALL == (1, 3) and R.FWD_N_MFMA == (4, 5, 6) and R.MEGA_T == (1, 32, 33)
    assert 2 * 3 % 4 == 2 and 2 * 5 % 4 == 2 and 2 * 4 % 4 == 0 and 2 * 6 % 4 == 0       # a tail of two rows at N = 3 and 5, a workgroup across
    assert 3 % 4 != 0 and 5 % 4 != 0 and 6 % 4 != 0                                         # the direction boundary at N = 3, 5 and 6
    lds = lambda T: 2 * T * (2 * 128 + 4) * 4
    assert lds(73) <= 150 * 1024 < lds(74)                                                 # T = 74 is the first the mega kernel refuses


def test_exact_forward_fixtures_have_integer_partial_sums_below_2_24_and_the_relu_edges():
    ab = lambda t: np.abs(np.asarray(t, np.float64))
    for seed in (0, 1):
        P = R.brain_params(seed, True)
        assert all(_is_integer(v) for v in P.values()) and not (P["encoder_fc1.bias"] == 0).any()
        for rows in R.ENC_ROWS:
            x = R.enc_fixture(rows, True, seed)
            a1, e, gx = R.enc(P, x)
            assert _is_integer(a1) and _is_integer(e) and _is_integer(gx), "a subnormal input reached a sum"
            m1 = ab(x) @ ab(P["encoder_fc1.weight"]).T + ab(P["encoder_fc1.bias"])
            m2 = m1 @ ab(P["encoder_fc2.weight"]).T + ab(P["encoder_fc2.bias"])
            assert (m2 @ ab(P["lstm_cell.weight_ih"]).T).max() < EXACT_LIMIT
            assert (a1 == 0).any() and (a1 > 0).any()
            if rows >= 6:
                assert (x == R.SUBNORMAL).any() and (x == -R.SUBNORMAL).any() and (x < -0.5).any()
                assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
            hs = R.dec_fixture(rows, True, seed)
            assert _is_integer(hs) and all(R.has_every_mask_class(r, integer=True) for r in hs)
            m = np.maximum(hs, 0).astype(np.float64) @ ab(P["decoder_fc1.weight"]).T + ab(P["decoder_fc1.bias"])
            assert (m @ ab(P["decoder_fc2.weight"])[0] + ab(P["decoder_fc2.bias"])[0]).max() < EXACT_LIMIT
            d1, _ = R.dec(P, hs)
            assert (d1 == 0).any() and (d1 > 0).any()


def test_dense_forward_fixtures_put_the_relu_on_its_edge():
    P = R.brain_params(0, False)
    assert not P["encoder_fc1.bias"][:4].any() and (P["encoder_fc1.bias"][4:] != 0).all()
    for rows in R.ENC_ROWS:
        x = R.enc_fixture(rows, False)
        a1, _, _ = R.enc(P, x)
        assert np.array_equal(a1[:, 0], np.maximum(x[:, 0], 0).astype(np.float64)) and np.array_equal(a1[:, 3], np.maximum(-x[:, 1], 0).astype(np.float64))
        assert (a1[:, :4] == R.SUBNORMAL).any()                      # the smallest subnormal passes the relu as itself
        if rows >= 6:
            assert sorted(set(a1[-6:, :4].ravel().tolist())) == [0.0, float(R.SUBNORMAL), 1.0, 2.0]
        assert all(R.has_every_mask_class(r) for r in R.dec_fixture(rows, False))
        b_a1, b_e, b_gx = R.enc_bounds(P, x)
        assert (b_a1[:, :4] <= 4 * R.U23 * float(np.abs(x).max())).all() and b_gx.max() < 1e-3 and b_gx.min() > 0


def test_recurrence_fixtures_saturate_and_bound_as_the_gpu_tests_assume():
    for N, T in ((3, 9), (5, 3)):
        whh, gx = R.saturating_fixture(N, T)
        signs = {tuple(bool(gx[n, t, k * 128 + j] > 0) for k in range(4)) for n in range(N) for t in range(T) for j in range(128)}
        assert len(signs) == 16 and (np.abs(gx) == 100).all()
        hs, gates, cs, hprev = R.lstm_fwd(whh, gx)
        pre = gx[None].astype(np.float64) + hprev @ whh.astype(np.float64).T
        assert np.abs(pre).min() >= 95, "exp2 of 95 log2(e) = 137 overflows fp32, of -137 vanishes beside 1"
        assert np.isfinite(hs).all() and np.abs(cs).max() <= T
    whh, gx = R.fwd_fixture(5, 9)
    a_s, a_g, a_c = R.act_terms(whh, gx)
    assert 0 < a_s < 2e-6 and 0 < a_g < 2e-6 and 0 < a_c < 2e-6           # a handful of fp32 ulps of numbers below 1
    hs, gates, cs, hprev = R.lstm_fwd(whh, gx)
    b_g, b_c, b_h = R.step_bounds(whh, gx[:, 4], hprev[0, :, 4], cs[0, :, 3], (a_s, a_g, a_c))
    assert b_g.min() >= a_s and b_g.max() < 1e-4 and b_c.max() < 1e-4 and b_h.max() < 1e-4
    x = np.array([-100.0, -3.0, -0.0, 0.0, 0.5, 3.0, 100.0], np.float32)
    assert np.abs(R.gate_act32(x, 1) - 1 / (1 + np.exp(-x.astype(np.float64)))).max() < 3e-7
    assert np.abs(R.gate_act32(x, 2) - np.tanh(x.astype(np.float64))).max() < 3e-7 and np.abs(R.cell_tanh32(x) - np.tanh(x.astype(np.float64))).max() < 3e-7
    assert R.gate_act32(x, 1)[[0, -1]].tolist() == [0.0, 1.0] and R.gate_act32(x, 2)[[0, -1]].tolist() == [-1.0, 1.0]
