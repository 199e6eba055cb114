"""ivosw_brain_topk_ragged (the ragged, masked top-k that takes the argmax's place under agent.candidates / agent.skip_annotated) on the
GPU: exact integer equality against the numpy restatement of its order in tests/test_topk_option.py, `qv` bit-equal to q[idx], and the
recommendation chain that ends in it (Agent.candidates_device, utils_agent.recommend_candidates, run_eval on the synthetic back end)."""
import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import entry, synth
from ivos_w_amd.models.agent import Agent, Brain
from ivos_w_amd.models.assessment import AssessNet
from ivos_w_amd.utils import utils_agent
from tests.test_topk_option import AD, rank_frames, topk_reference

pytestmark = pytest.mark.gpu

# the wave strides 64 frames: one trip, the edge of one, two and three trips; 15 / 16 / 17 around k = 16; 256 / 257: the last length whose
# keys stay in registers and the first that is rescanned from memory every round (300: several trips of that path).  Mixed in one call,
# so every sequence but the first starts at an unaligned row.
LENGTHS = [1, 2, 63, 64, 65, 127, 129, 15, 16, 17, 256, 257, 300]
KS = [1, 2, 16]                    # k = T and k = T + 1 occur at T = 1, 2, 15, 16: the -1 fill


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _topk(dev, q, counts, lengths, k, skip, with_state=True):
    """The C entry on host arrays: (idx [K, k], qv [K, k]) with one guard row behind each checked."""
    K, R = len(lengths), sum(lengths)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    sd = None
    if with_state:
        st = np.stack([np.full(R, 0.5, dtype=np.float32), np.asarray(counts, dtype=np.float32)], 1)
        sd = torch.from_numpy(st).to(dev)
    idx = torch.full((K + 1, k), -7, dtype=torch.int64, device=dev)
    qv = torch.full((K + 1, k), -7.5, dtype=torch.float32, device=dev)
    L.check(L.lib().ivosw_brain_topk_ragged(L.dptr(qd), L.dptr(sd) if sd is not None else None, L.int_array(lengths), K, k, int(skip), L.dptr(idx),
                                            L.dptr(qv), L.stream_ptr(dev)), "topk_ragged")
    idx, qv = idx.cpu().numpy(), qv.cpu().numpy()
    assert (idx[K] == -7).all() and (qv[K] == -7.5).all()
    return idx[:K], qv[:K]


def _check(dev, q, counts, lengths, k, skip, **kw):
    q = np.asarray(q, dtype=np.float32)
    idx, qv = _topk(dev, q, counts, lengths, k, skip, **kw)
    want_idx, want_qv = topk_reference(q, counts, lengths, k, skip)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(qv.view(np.int32), want_qv.view(np.int32))       # the bits of q[idx] (NaN payloads, the sign of zero)
    return idx


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)])


def _scenario(name, lengths, k):
    """(q, counts) over the flat rows of `lengths`."""
    rs = np.random.RandomState(len(name) * 131 + k)
    R, offs = sum(lengths), _offsets(lengths)
    q = rs.randn(R).astype(np.float32)
    counts = np.zeros(R, dtype=np.float32)
    rows = [(int(o), n) for o, n in zip(offs[:-1], lengths)]
    if name == "random_none_annotated":
        pass
    elif name == "random_some_annotated":
        counts = rs.randint(0, 3, R).astype(np.float32)
    elif name == "all_annotated":                                      # falls through to the annotated tier
        counts = rs.randint(1, 4, R).astype(np.float32)
    elif name == "one_left_and_it_is_the_worst":
        counts[:] = 1
        for o, n in rows:
            t = int(rs.randint(n))
            q[o + t] = -50.0
            counts[o + t] = 0
    elif name == "annotated_hold_the_best":
        for o, n in rows:
            best = np.argsort(-q[o:o + n], kind="stable")[:k]
            counts[o + best] = 2
    elif name == "all_equal":
        q[:] = 0.75
        counts = rs.randint(0, 2, R).astype(np.float32)
    elif name == "few_values_many_ties":
        q = rs.randint(0, 3, R).astype(np.float32)
        counts = rs.randint(0, 2, R).astype(np.float32)
    elif name == "equal_maxima":
        for o, n in rows:
            if n > 64:                                                  # t and t + 64: one lane in two trips
                q[o + 3] = q[o + 67] = 9.0
            if n > 41:                                                  # t and t + 1: neighbouring lanes
                q[o + 40] = q[o + 41] = 8.0
    elif name == "signed_zeros_and_infinities":
        q = -np.abs(q)
        for o, n in rows:
            if n >= 2:
                q[o + n - 1], q[o + n - 2] = 0.0, -0.0                  # -0.0 before +0.0, at equal rank, on top
            if n > 20:
                q[o + 5], q[o + 9], q[o + 13], q[o + 17] = np.inf, -np.inf, np.inf, -np.inf
        counts = (rs.rand(R) < 0.3).astype(np.float32)
    elif name == "nans":
        for i, (o, n) in enumerate(rows):
            if i % 4 == 0:
                q[o] = np.nan                                           # one NaN, at index 0
            elif i % 4 == 1:
                q[o:o + n] = np.nan                                     # a row that is all NaN
            elif i % 4 == 2:
                q[o + rs.choice(n, size=max(1, n // 3), replace=False)] = np.nan
                q[o] = np.nan
            else:
                q[o + n - 1] = -np.nan                                  # the other sign bit
        counts = (rs.rand(R) < 0.4).astype(np.float32)
    else:
        raise KeyError(name)
    return q, counts


SCENARIOS = ["random_none_annotated", "random_some_annotated", "all_annotated", "one_left_and_it_is_the_worst", "annotated_hold_the_best",
             "all_equal", "few_values_many_ties", "equal_maxima", "signed_zeros_and_infinities", "nans"]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENARIOS)
def test_topk_equals_the_restated_order(dev, name, k):
    q, counts = _scenario(name, LENGTHS, k)
    offs = _offsets(LENGTHS)
    masked = _check(dev, q, counts, LENGTHS, k, True)
    _check(dev, q, counts, LENGTHS, k, False)
    _check(dev, q, None, LENGTHS, k, False, with_state=False)           # no state at all with the flag clear
    for s, (o, n) in enumerate(zip(offs[:-1], LENGTHS)):
        got = masked[s][masked[s] >= 0]
        assert len(got) == min(k, n) and len(set(got.tolist())) == len(got) and (masked[s][min(k, n):] == -1).all()
        if name == "one_left_and_it_is_the_worst":
            assert counts[o + got[0]] == 0 and q[o + got[0]] == -50.0
        if name == "annotated_hold_the_best" and n >= 2 * k:
            assert (counts[o + got] == 0).all()
        if name == "all_equal" and n > 1 and counts[o:o + n].min() == counts[o:o + n].max():
            assert got.tolist() == list(range(min(k, n)))               # ascending in index


@pytest.mark.parametrize("n_seqs", [1, 2, 128])
def test_topk_for_one_two_and_128_sequences(dev, n_seqs):
    rs = np.random.RandomState(n_seqs)
    lengths = {1: [65], 2: [129, 1], 128: [1 + (7 * s) % 70 for s in range(128)]}[n_seqs]
    R = sum(lengths)
    q = rs.randint(0, 40, R).astype(np.float32) / 8                     # some ties
    counts = rs.randint(0, 2, R).astype(np.float32)
    for k in KS:
        _check(dev, q, counts, lengths, k, True)
        _check(dev, q, counts, lengths, k, False)
    if n_seqs == 1:                                                     # k = T and k = T + 1 on a single sequence
        for T, k in ((1, 1), (1, 2), (2, 2), (16, 16), (15, 16), (64, 16)):
            got = _check(dev, q[:T], counts[:T], [T], k, True)
            assert (got[0, :min(T, k)] >= 0).all() and (got[0, min(T, k):] == -1).all()


def test_topk_with_one_candidate_is_the_ragged_argmax(dev):
    rs = np.random.RandomState(8)
    lengths = LENGTHS + [130, 70]
    K, R = len(lengths), sum(lengths)
    for q in (rs.randn(R).astype(np.float32), rs.randint(0, 4, R).astype(np.float32)):       # tie-free, and with many equal maxima
        idx, _ = _topk(dev, q, None, lengths, 1, False, with_state=False)
        ref = torch.full((K,), -1, dtype=torch.int64, device=dev)
        L.check(L.lib().ivosw_brain_argmax_ragged(L.dptr(torch.from_numpy(q).to(dev)), L.int_array(lengths), K, L.dptr(ref), L.stream_ptr(dev)),
                "argmax_ragged")
        assert idx[:, 0].tolist() == ref.cpu().tolist()
        offs = _offsets(lengths)
        assert idx[:, 0].tolist() == [int(np.argmax(q[o:o + n])) for o, n in zip(offs[:-1], lengths)]


def _agent(dev, phase="eval", **options):
    cfg = AD(phase=phase, data=AD(subset="val"), agent=AD(memory_size=100, gamma=0.95, eps_start=0.7, eps_end=0.25, eps_decay=500,
                                                          update_rate=0.05, lr=5e-6, weight_decay=5e-4, **options))
    agent = Agent(dev, cfg)
    agent.policy_net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.brain_state_dict(0).items()})
    return agent


def test_agent_topk_ragged_groups_more_than_128_sequences(dev):
    agent = _agent(dev)
    rs = np.random.RandomState(4)
    lengths = [1 + (5 * s) % 9 for s in range(131)]
    R, k = sum(lengths), 4
    q = rs.randint(0, 12, R).astype(np.float32)
    counts = rs.randint(0, 2, R).astype(np.float32)
    qd = torch.from_numpy(q).to(dev)
    sd = torch.from_numpy(np.stack([q, counts], 1)).to(dev)
    want_idx, want_qv = topk_reference(q, counts, lengths, k, True)
    qv = torch.full((131, k), -7.5, dtype=torch.float32, device=dev)
    idx = agent.topk_ragged(qd, sd, lengths, k, True, qv=qv)
    assert idx.shape == (131, k) and idx.dtype == torch.int64
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(qv.cpu().numpy().view(np.int32), want_qv.view(np.int32))
    out = torch.full((131 * k + 1,), -7, dtype=torch.int64, device=dev)   # a flat caller buffer, as the recommendation chain passes it
    agent.topk_ragged(qd, None, lengths, k, False, out=out[:131 * k])
    np.testing.assert_array_equal(out[:131 * k].view(131, k).cpu().numpy(), topk_reference(q, None, lengths, k, False)[0])
    assert int(out[-1]) == -7
    with pytest.raises(RuntimeError, match="skip_annotated"):
        agent.topk_ragged(qd, None, lengths, k, True)


# ---------------------------------------------------------------------------------------------- the recommendation chain
class _Vid:
    def __init__(self, dev, g, n, O, H=120, W=216):                     # the synthetic session's frame size
        self.frames, self.all_P, self.O, self.n = torch.rand(n, 3, H, W, generator=g).to(dev), torch.rand(n, O + 1, H, W, generator=g).to(dev), O, n


@pytest.fixture(scope="module")
def assess(dev):
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()}, strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope="module")
def videos(dev):
    g = torch.Generator().manual_seed(99)
    return [_Vid(dev, g, 6, 2), _Vid(dev, g, 9, 1), _Vid(dev, g, 5, 3)]


def _requests(vids, annotated):
    return [dict(n_frame=v.n, n_objects=v.O, all_F=v.frames, all_P=v.all_P, new_masks_quality=np.zeros(v.n), prev_frames=sorted(set(a)),
                 annotated_frames_list=list(a), mask_quality=np.zeros(v.n), first_frame=a[0], max_nb_interactions=8) for v, a in zip(vids, annotated)]


def _restated(agent, req, k, skip):
    """The restatement applied to Brain.forward's Q of the state the chain builds: (float32(quality), annotation counts)."""
    counts = utils_agent._annotation_counts(req["n_frame"], req["annotated_frames_list"])
    state = np.stack([req["mask_quality"].astype(np.float32), counts.astype(np.float32)], 1)
    q = agent.policy_net(torch.from_numpy(state).to(agent.device)[None])[0].cpu().numpy()
    return rank_frames(q, counts, skip)[:k]


@pytest.mark.parametrize("n_sessions", [2, 3])
def test_recommend_candidates_is_one_ragged_chain_that_ends_in_the_topk(dev, assess, videos, monkeypatch, n_sessions):
    vids = videos[:n_sessions]
    annotated = [[1, 1, 0], [4, 2, 4, 7], [3]][:n_sessions]
    cy = AD(setting="wild", method="ours")
    plain, agent = _agent(dev), _agent(dev, candidates=3, skip_annotated=True)
    want_req = _requests(vids, annotated)
    want = [int(i) for i in utils_agent.recommend_frames(cy, assess, plain, dev, want_req)]
    got_req = _requests(vids, annotated)
    calls = []
    real_cpu, real_item, real_fwd, real_ragged = torch.Tensor.cpu, torch.Tensor.item, Brain.forward, Brain.forward_ragged
    real_topk, real_argmax = Agent.topk_ragged, Agent.argmax_ragged
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(Brain, "forward", lambda self, *a, **k: (calls.append("forward"), real_fwd(self, *a, **k))[1])
    monkeypatch.setattr(Brain, "forward_ragged", lambda self, *a, **k: (calls.append("forward_ragged"), real_ragged(self, *a, **k))[1])
    monkeypatch.setattr(Agent, "topk_ragged", lambda self, *a, **k: (calls.append("topk_ragged"), real_topk(self, *a, **k))[1])
    monkeypatch.setattr(Agent, "argmax_ragged", lambda self, *a, **k: (calls.append("argmax_ragged"), real_argmax(self, *a, **k))[1])
    got = utils_agent.recommend_candidates(cy, assess, agent, dev, got_req)
    monkeypatch.undo()
    # ONE ragged forward (three launches) and ONE top-k launch behind the quality -> state launch, ONE device-to-host copy, no argmax
    assert sorted(calls) == ["cpu", "forward_ragged", "topk_ragged"], calls
    for a, b in zip(got_req, want_req):
        np.testing.assert_array_equal(a["mask_quality"].view(np.int64), b["mask_quality"].view(np.int64))
        assert np.ptp(a["mask_quality"]) > 0
    for c, r, v in zip(got, got_req, vids):
        assert isinstance(c, np.ndarray) and c.dtype == np.int64 and len(c) == min(3, v.n)
        assert c.tolist() == _restated(agent, r, 3, True).tolist()
        if len(set(r["annotated_frames_list"])) < v.n:
            assert int(c[0]) not in r["annotated_frames_list"]
    # recommend_frames under the options returns candidate 0; with both at their defaults recommend_candidates is recommend_frames
    assert [int(i) for i in utils_agent.recommend_frames(cy, assess, agent, dev, _requests(vids, annotated))] == [int(c[0]) for c in got]
    same = utils_agent.recommend_candidates(cy, assess, plain, dev, _requests(vids, annotated))
    assert [c.tolist() for c in same] == [[i] for i in want]
    assert want == [int(_restated(plain, r, 1, False)[0]) for r in want_req]
    assert agent.steps_done == 2 * n_sessions and plain.steps_done == 2 * n_sessions


def test_recommend_candidates_with_every_frame_but_one_annotated(dev, assess, videos):
    cy = AD(setting="wild", method="ours")
    agent = _agent(dev, candidates=3, skip_annotated=True)
    left = [4, 0, 2]
    annotated = [[t for t in range(v.n) if t != keep] for v, keep in zip(videos, left)]
    got = utils_agent.recommend_candidates(cy, assess, agent, dev, _requests(videos, annotated))
    assert [int(c[0]) for c in got] == left and all(len(c) == 3 and len(set(c.tolist())) == 3 for c in got)
    one = _agent(dev, skip_annotated=True)                              # one candidate: the same types as today, that frame
    picks = utils_agent.recommend_frames(cy, assess, one, dev, _requests(videos, annotated))
    assert [int(i) for i in picks] == left and all(isinstance(i, np.int64) for i in picks)
    # one request: the per-request chain (Brain.forward and a one-sequence top-k), the same candidates
    utils_agent.clear_frame_cache()
    for v, a, c in zip(videos, annotated, got):
        req = _requests([v], [a])
        single = utils_agent.recommend_candidates(cy, assess, agent, dev, req)
        assert len(single) == 1 and single[0].tolist() == c.tolist() == _restated(agent, req[0], 3, True).tolist()
        assert int(utils_agent.recommend_frame(cy, assess, agent, dev, **_requests([v], [a])[0])) == int(c[0])
    utils_agent.clear_frame_cache()


def test_run_eval_submits_distinct_candidates_and_skips_annotated_frames(dev, tmp_path, monkeypatch):
    cfg = entry.parse_cli(["with", "synthetic=1", "setting=wild", "method=ours", "synth.n_sequences=1", "synth.n_frames=8", "synth.height=48",
                           "synth.width=80", "eval_max_nb_interactions=7", "agent.candidates=3", "agent.skip_annotated=true",
                           "davis_interactive.allow_repeat=0", f"ckpt_dir={tmp_path}/weights", f"report_save_dir={tmp_path}/results"])
    seen, submitted = [], []
    real_rec, real_submit = utils_agent.recommend_candidates, entry.SyntheticSession.submit_masks

    def rec(cfg_yl, assess_net, agent, device, requests):
        seen.append(list(requests[0]["prev_frames"]))
        return real_rec(cfg_yl, assess_net, agent, device, requests)

    def submit(self, masks, next_scribble_frame_candidates=None):
        submitted.append(list(next_scribble_frame_candidates))
        return real_submit(self, masks, next_scribble_frame_candidates=next_scribble_frame_candidates)
    monkeypatch.setattr(utils_agent, "recommend_candidates", rec)
    monkeypatch.setattr(entry.SyntheticSession, "submit_masks", submit)
    utils_agent.clear_frame_cache()
    out = entry.run_eval(cfg, "MANet")
    utils_agent.clear_frame_cache()
    assert out["backend"] == "synthetic" and len(submitted) == len(seen) and len(submitted) >= 7
    for prev, cand in zip(seen, submitted):
        assert len(cand) == 3 and len(set(cand)) == 3 and all(isinstance(i, int) and 0 <= i < 8 for i in cand)
        assert len(set(prev)) < 8 and cand[0] not in prev              # (at most 7 of the 8 frames are ever annotated)
