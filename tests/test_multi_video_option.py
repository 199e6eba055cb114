"""Multi-video assessment, the parts that need no GPU: the host-side unit count and refusals of the C ABI, recommend_frames' fall-back
to recommend_frame for every setting / method without an assessment pass, and forward_videos' refusals."""
import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd.models.assessment import AssessNet
from ivos_w_amd.utils import utils_agent


class AD(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _videos(*rows):
    """L.Video array from (kind, n_frames, n_obj, H, W) rows; the pointers are made-up, aligned addresses that nothing dereferences."""
    arr = (L.Video * len(rows))()
    for v, (kind, n, o, H, W) in zip(arr, rows):
        v.frames, v.masks, v.mask_stride_frame, v.mask_stride_obj = 0x10000, 0x20000, (o + 1) * H * W, H * W
        v.frames_kind, v.n_frames, v.n_obj, v.H, v.W = kind, n, o, H, W
    return arr


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_units_is_the_sum_over_the_videos(lib):
    assert L.MAX_VIDEOS == 32
    assert lib.ivosw_assess_videos_units(_videos((0, 3, 2, 40, 56), (0, 2, 1, 37, 51), (1, 1, 3, 33, 47), (0, 1, 1, 2, 2)), 4) == 12
    assert lib.ivosw_assess_videos_units(_videos(*[(1, 1, 1, 2, 2)] + [(0, 5, 7, 480, 854)] * 31), 32) == 1 + 31 * 35
    assert lib.ivosw_assess_videos_units(_videos((0, 1 << 15, (1 << 15) - 1, 2, 2)), 1) == (1 << 30) - (1 << 15)


def test_host_side_refusals_name_the_video(lib):
    msg = lambda: lib.ivosw_last_error().decode()
    good = [(0, 3, 2, 40, 56), (1, 2, 1, 37, 51), (0, 4, 1, 8, 8)]

    def refused(arr, n, *words):
        assert lib.ivosw_assess_videos_units(arr, n) == -1
        assert all(w in msg() for w in words), msg()
        # the launching entries refuse the same array before they look at anything else (NULL outputs are never reached)
        assert lib.ivosw_mask_bbox_videos(arr, n, None, None, None) == -1 and all(w in msg() for w in words)
        assert lib.ivosw_roi_sample_videos(arr, n, None, L.F32, None, None) == -1 and all(w in msg() for w in words)
        assert lib.ivosw_assess_forward_videos(None, L.BF16, arr, n, None, None, 0, 0, 0, None, None) == -1 and all(w in msg() for w in words)
    refused(None, 1, "null pointer")
    for n in (0, -2, 33):
        refused(_videos(*good), n, "n_videos", str(n))
    for i, field, value, word in [(0, "frames", None, "null pointer"), (2, "masks", None, "null pointer"), (1, "frames_kind", 2, "frames_kind"),
                                  (0, "n_frames", 0, "positive"), (2, "n_obj", -1, "positive"), (1, "H", 1, "H, W > 1"), (2, "W", 1, "H, W > 1"),
                                  (0, "mask_stride_frame", -1, "negative"), (1, "mask_stride_obj", -1, "negative"),
                                  (0, "mask_stride_frame", 40 * 56 - 1, "overlap"), (1, "frames", 0x10002, "4-byte aligned")]:
        arr = _videos(*good)
        setattr(arr[i], field, value)
        refused(arr, 3, f"video {i}", word)
    arr = _videos(*good)
    arr[2].H, arr[2].W, arr[2].n_frames = 65536, 32768, 1
    refused(arr, 3, "video 2", "INT_MAX")
    arr = _videos((0, 1 << 15, 1 << 14, 2, 2), (0, 1 << 15, 1 << 14, 2, 2), (0, 1, 1, 2, 2))
    refused(arr, 3, "video 1", "too many")                                     # 2^30 units are reached at the second video
    assert lib.ivosw_assess_videos_units(arr, 1) == 1 << 29
    # an fp32 video may sit at any 4-byte address; a single frame may have any frame stride
    arr = _videos(*good)
    arr[0].frames, arr[2].n_frames, arr[2].mask_stride_frame = 0x10004, 1, 0
    assert lib.ivosw_assess_videos_units(arr, 3) == 6 + 2 + 1


# ---------------------------------------------------------------------------------------------- recommend_frames without an assessment pass
class _Agent:
    """Stands in for models.agent.Agent under oracle/ours: a deterministic pick from the state, and the step count."""

    def __init__(self):
        self.steps_done, self.states = 0, []

    def action(self, state):
        self.steps_done += 1
        self.states.append(np.array(state))
        return int(np.argmin(state[:, 0] + 0.01 * state[:, 1]))


def _requests(seed):
    rs = np.random.RandomState(seed)
    out = []
    for n in (7, 12, 5):
        out.append(dict(n_frame=n, n_objects=2, all_F=None, all_P=None, new_masks_quality=rs.rand(n), prev_frames=[0, n // 2],
                        annotated_frames_list=[0, n // 2, 0], mask_quality=np.zeros(n), first_frame=0, max_nb_interactions=4))
    return out


@pytest.mark.parametrize("setting,method", [("oracle", "worst"), ("oracle", "ours"), ("wild", "random"), ("wild", "linspace")])
def test_recommend_frames_falls_back_to_recommend_frame(setting, method):
    cfg = AD(setting=setting, method=method)
    a, b = _Agent(), _Agent()
    np.random.seed(11)
    want = [utils_agent.recommend_frame(cfg, None, a, "cpu", **r) for r in _requests(4)]
    after_want = np.random.rand()
    np.random.seed(11)
    got = utils_agent.recommend_frames(cfg, None, b, "cpu", _requests(4))
    assert [int(v) for v in got] == [int(v) for v in want]
    assert np.random.rand() == after_want                                      # the same np.random stream
    assert a.steps_done == b.steps_done == (3 if (setting, method) == ("oracle", "ours") else 0)
    assert all(np.array_equal(x, y) for x, y in zip(a.states, b.states))
    assert utils_agent.recommend_frames(cfg, None, b, "cpu", []) == []


def test_recommend_frames_keeps_unknown_methods_loud():
    with pytest.raises(NotImplementedError):
        utils_agent.recommend_frames(AD(setting="wild", method="nope"), None, None, "cpu", _requests(1))


# ---------------------------------------------------------------------------------------------- forward_videos' refusals
def test_forward_videos_refuses_training_mode_and_a_cpu_network():
    net = AssessNet()
    video = (torch.zeros(2, 3, 16, 16), torch.zeros(2, 2, 16, 16), 1)
    with pytest.raises(RuntimeError, match="inference-only"):
        net.train().forward_videos([video])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval().forward_videos([video])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval().forward_objects(*video)                                     # as loudly as the single-video entry
    assert net.eval().forward_videos([]) == []
