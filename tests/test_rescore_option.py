"""Incremental assessment (rescore=all|changed), without a GPU: the option parses and refuses like ``frames``, the header and the binding
declare the five entries, a ScoreCache goes cold on every component of its key, the score-cache LRU evicts by bytes, and the default path
never constructs a cache."""
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry
from ivos_w_amd.models import assessment
from ivos_w_amd.models.assessment import PackedFrames, ScoreCache
from ivos_w_amd.utils import utils_agent


class StubNet:
    """What the cache key reads of an AssessNet, and a forward that needs no device."""

    def __init__(self, precision="bf16", wkey=("w", 0)):
        self.precision, self.wkey, self.calls = precision, wkey, []

    def _weights_key(self):
        return (self.precision,) + tuple(self.wkey)

    def forward_objects(self, frames, probs, n_objects):
        self.calls.append("forward_objects")
        return torch.zeros(n_objects, frames.shape[0])

    def forward_videos(self, videos):
        self.calls.append("forward_videos")
        return [torch.zeros(o, f.shape[0]) for f, _, o in videos]

    def forward_videos_incremental(self, videos, caches, sources=None):
        self.calls.append("forward_videos_incremental")
        for (f, _, o), c, s in zip(videos, caches, sources):
            c.bind(self, s, f.shape[0], o, f.shape[2], f.shape[3], "cpu")
            c._rescored = c.units
        return [torch.zeros(o, f.shape[0]) for f, _, o in videos]


# ---------------------------------------------------------------------------------------------- the option
def test_rescore_parses_defaults_to_all_and_refuses_other_values(tmp_path):
    assert entry.DEFAULTS["rescore"] == "all"
    assert entry.parse_cli([]).rescore == "all"
    assert entry.parse_cli(["with", "rescore=changed"]).rescore == "changed"
    assert entry.parse_cli(["with", "rescore=all"]).rescore == "all"
    y = tmp_path / "c.yaml"
    y.write_text("rescore: changed\n")
    assert entry.parse_cli(["--config", str(y)]).rescore == "changed"
    for bad in ("dirty", "CHANGED", "All", "1", "true", "none", ""):
        with pytest.raises(SystemExit, match="rescore"):
            entry.parse_cli(["with", f"rescore={bad}"])
    with pytest.raises(SystemExit, match="rescore"):
        entry.parse_cli([], rescore=1)
    # read with .get: a config written before the key existed scores everything; run_eval refuses a bad value before any work
    assert entry.rescore_option({}) == "all" and entry.rescore_option(dict(rescore="changed")) == "changed"
    assert utils_agent.rescore_option(None) == "all"
    cfg = entry.parse_cli(["with", "synthetic=1"])
    cfg.rescore = "some"
    with pytest.raises(ValueError, match="rescore"):
        entry.run_eval(cfg)
    assert utils_agent.RESCORE_MODES == ("all", "changed") and utils_agent.SCORE_CACHE_BYTES == 8 << 30


def test_binding_declares_the_entries():
    S = L.SIGNATURES
    assert S["ivosw_mask_delta_videos"] == (L._i, [L._p, L._i, L._p, L._p, L._p, L._p, L._p, L._p])
    assert S["ivosw_mask_bbox_units"] == (L._i, [L._p, L._i, L._p, L._i, L._p, L._p, L._p])
    assert S["ivosw_roi_sample_units"] == (L._i, [L._p, L._i, L._p, L._i, L._p, L._i, L._p, L._p])
    assert S["ivosw_assess_units_ws_bytes"] == (L._sz, [L._i, L._i, L._i])
    assert S["ivosw_assess_forward_units"] == (L._i, [L._p, L._i, L._p, L._i, L._p, L._i, L._p, L._p, L._sz, L._i, L._p])
    if L.available():                                   # host-only query: a pass of n units plus the compact [n] score buffer
        lib = L.lib()
        assert lib.ivosw_assess_units_ws_bytes(L.BF16, 0, 0) == 0 and lib.ivosw_assess_units_ws_bytes(L.BF16, -3, 0) == 0
        assert lib.ivosw_assess_units_ws_bytes(7, 5, 0) == 0
        for n in (1, 5, 70):
            assert lib.ivosw_assess_units_ws_bytes(L.BF16, n, 0) == lib.ivosw_assess_ws_bytes(L.BF16, n, 2, 2, 0) + (4 * n + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------- ScoreCache
def test_score_cache_goes_cold_on_every_key_component():
    net = StubNet()
    frames = torch.zeros(4, 3, 6, 8)
    c = ScoreCache()
    assert c.nbytes == 0
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is True                      # first sight: cold
    assert c.units == 8 and tuple(c.scores.shape) == (2, 4) and c.planes.numel() == 8 * 48
    assert c.nbytes == ScoreCache.nbytes_for(4, 2, 6, 8) == 4 * 8 * 49
    assert c.src is frames                                                     # a strong reference, as _FrameCache holds its tensor
    planes = c.planes
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is False and c.planes is planes
    twin = torch.zeros(4, 3, 6, 8)                                             # equal content, another object
    assert c.bind(net, twin, 4, 2, 6, 8, "cpu") is True
    assert c.bind(net, twin, 4, 2, 6, 8, "cpu") is False
    twin.add_(1.0)                                                             # rewritten through torch: the version moves
    assert c.bind(net, twin, 4, 2, 6, 8, "cpu") is True
    frames = twin
    for dims in ((3, 2, 6, 8), (4, 1, 6, 8), (4, 2, 5, 8), (4, 2, 6, 7)):      # n_frames, n_obj, H, W
        assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is False
        assert c.bind(net, frames, *dims, "cpu") is True
        assert c.planes.numel() == dims[0] * dims[1] * dims[2] * dims[3]
        assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is True
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is False
    assert c.bind(StubNet(precision="fp32"), frames, 4, 2, 6, 8, "cpu") is True
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is True
    net.wkey = ("w", 1)                                                        # the weights changed
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is True
    assert c.bind(net, frames, 4, 2, 6, 8, "cpu") is False
    pf = PackedFrames(torch.zeros(4, 6, 8, 4, dtype=torch.uint8))
    assert c.bind(net, pf, 4, 2, 6, 8, "cpu") is True and c.src is pf
    assert c.bind(net, pf, 4, 2, 6, 8, "cpu") is False
    c.clear()
    assert c.key is None and c.src is None and c.planes is None and c.nbytes == 0
    assert c.bind(net, pf, 4, 2, 6, 8, "cpu") is True


# ---------------------------------------------------------------------------------------------- the LRU
def test_lru_evicts_by_bytes(monkeypatch):
    lru = utils_agent._ScoreCacheLRU()
    net = StubNet()
    vids = [torch.zeros(2, 3, 4, 5) for _ in range(4)]
    one = ScoreCache.nbytes_for(2, 1, 4, 5)
    monkeypatch.setattr(utils_agent, "SCORE_CACHE_BYTES", 2 * one)

    def use(*idx):
        on_dev = [(vids[i], None, 1) for i in idx]
        caches = lru.get_many(net, on_dev)
        net.forward_videos_incremental(on_dev, caches, sources=[vids[i] for i in idx])
        lru.account(caches)
        return caches
    (c0,) = use(0)
    (c1,) = use(1)
    assert lru.nbytes() == 2 * one and len(lru.entries) == 2
    assert use(0) == [c0] and c0.key is not None                               # found again, and now the most recent
    (c2,) = use(2)                                                             # over the limit: the least recently used (video 1) goes
    assert len(lru.entries) == 2 and lru.nbytes() == 2 * one
    assert c1.key is None and c1.planes is None and c0.key is not None and c2.key is not None
    assert use(0) == [c0]
    (c1b,) = use(1)                                                            # a new cache for video 1; video 2 goes
    assert c1b is not c1 and c2.key is None and c0.key is not None
    # two videos of one call on ONE frames object get a cache each
    a, b = use(3, 3)
    assert a is not b and len(lru.entries) == 2
    assert lru.stats() == (2 * 8, 2 * 8)                                       # 6 single-video calls and one of two videos, 2 units each, all scored (the stub)
    lru.trim(0)
    assert not lru.entries and a.key is None
    lru.clear()
    assert lru.stats() == (0, 0)


def test_clear_score_cache_drops_everything():
    net = StubNet()
    v = torch.zeros(2, 3, 4, 5)
    (c,) = utils_agent.score_cache.get_many(net, [(v, None, 1)])
    c.bind(net, v, 2, 1, 4, 5, "cpu")
    assert utils_agent.score_cache.entries
    utils_agent.clear_score_cache()
    assert not utils_agent.score_cache.entries and c.key is None and c.src is None


# ---------------------------------------------------------------------------------------------- the default path
def test_default_path_never_constructs_a_cache(monkeypatch):
    made = []
    real = ScoreCache.__init__
    monkeypatch.setattr(assessment.ScoreCache, "__init__", lambda self: (made.append(1), real(self))[1])
    utils_agent.clear_score_cache()
    utils_agent.clear_frame_cache()
    net = StubNet()
    F, P = torch.zeros(3, 3, 4, 5), torch.zeros(3, 2, 4, 5)
    out = utils_agent.assess_all_objects_device(net, F, P, 1, "cpu")
    assert tuple(out.shape) == (1, 3)
    assert tuple(utils_agent.assess_all_objects(net, F, P, 1, "cpu").shape) == (3, 1)
    utils_agent.assess_videos_device(net, [(F, P, 1)], "cpu")
    assert net.calls == ["forward_objects", "forward_objects", "forward_videos"] and not made
    assert not utils_agent.score_cache.entries
    # ... and the opt-in goes through the incremental forward and the cache
    utils_agent.assess_all_objects_device(net, F, P, 1, "cpu", rescore="changed")
    utils_agent.assess_videos_device(net, [(F, P, 1)], "cpu", rescore="changed")
    assert net.calls[3:] == ["forward_videos_incremental"] * 2 and made == [1]
    assert utils_agent.score_cache.stats() == (6, 6)
    utils_agent.clear_score_cache()
    utils_agent.clear_frame_cache()
