"""GPU: a three-interaction IPN session driven through utils_ipn (Dilate_mask, Get_weight, merge_round, To_np_label, IpnStore) - 7
frames, two objects (K = 3 channels), 12 x 20 - against the same loop written with torch CPU and numpy ops: the reference's host
functions restated (tests/ipn_ref.py) and the per-frame blend (w * new) + ((1 - w) * old) with Python scalars, as torch rounds it.

The model double returns seeded estimates of the right shape (they do not depend on what it is handed, so both loops see the same
estimates).  Nothing here is approximate: labels, merged estimate and all_P must be equal bit for bit."""
import numpy as np
import pytest
import torch

from ivos_w_amd import synth
from ivos_w_amd.models.assessment import AssessNet, LabelMasks
from ivos_w_amd.utils import utils_ipn as ui
from tests import ipn_ref as ir

pytestmark = pytest.mark.gpu

T, O, H, W = 7, 2, 12, 20
K = O + 1
TARGETS = (3, 0, 5)                                       # the annotated frame of each interaction
AT_LEAST = 2
PERMUTED = [2, 0, 1]                                      # index[j] = the canonical channel at position j


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class Model:
    """Seeded estimates, one draw per call: two Models answer the same sequence of calls with the same values."""

    def __init__(self, device):
        self.g = torch.Generator().manual_seed(412)
        self.device = device
        self.seen = []

    def Run(self, scribble_planes):
        self.seen.append(scribble_planes)
        e = torch.softmax(torch.randn(1, K, T, H, W, generator=self.g) * 2, dim=1)
        return e.to(self.device)


def _scribble(it):
    """A sparse indexed scribble map of interaction `it`: -1 = ignore, 0 = background, 1 .. O = the objects."""
    rng = np.random.default_rng(50 + it)
    m = -np.ones((H, W), np.int64)
    for o in range(O + 1):
        y, x = rng.integers(0, H), rng.integers(0, W - 5)
        m[y, x:x + 5] = o
    m[0, 0], m[H - 1, W - 1] = O, 0
    return m


def host_loop(index):
    """The loop with the reference's host code restated: the literal dilation loop, Get_weight, the per-frame torch blend, To_np_label,
    all_P = probs[0].transpose(1, 0) with probs in canonical channel order."""
    model = Model("cpu")
    prev_E, prev_targets, rounds = None, [], []
    inv_index = [index.index(i) for i in range(K)]
    for it, target in enumerate(TARGETS):
        dil = ir.dilate_ref(_scribble(it), O)
        all_E = model.Run(dil)
        raw = all_E.clone()
        if prev_E is not None:
            _, _, weight = ui.Get_weight(target, prev_targets, T, at_least=AT_LEAST)
            for f in range(T):
                all_E[:, :, f] = (weight[f] * all_E[:, :, f]) + ((1 - weight[f]) * prev_E[:, :, f])
        labels = ir.labels_ref(all_E[0].numpy(), index)
        probs = all_E[:, inv_index]
        rounds.append(dict(dil=dil, raw=raw, E=all_E.clone(), labels=labels, all_P=probs[0].transpose(1, 0).clone()))
        prev_E = all_E
        prev_targets.append(target)
    return rounds


def device_loop(dev, index, store):
    model = Model(dev)
    prev_E, prev_targets, rounds = None, [], []
    for it, target in enumerate(TARGETS):
        dil = ui.Dilate_mask(_scribble(it), O, device=dev)
        all_E = model.Run(dil)
        weight = None
        if prev_E is not None:
            _, _, weight = ui.Get_weight(target, prev_targets, T, at_least=AT_LEAST)
        final_masks, all_P = ui.merge_round(all_E, prev_E, weight, index, store)
        rounds.append(dict(dil=dil, E=all_E, labels=ui.To_np_label(all_E, K, index), final_masks=final_masks.clone(),
                           labels_u8=store.labels_u8.clone(), all_P=all_P if isinstance(all_P, LabelMasks) else all_P.clone(), live_all_P=all_P))
        prev_E = all_E
        prev_targets.append(target)
    return rounds


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("index", [list(range(K)), PERMUTED], ids=["identity", "permuted"])
def test_three_interactions_against_the_host_loop(dev, index):
    want = host_loop(index)
    store = ui.IpnStore(T, K, H, W, dev)
    got = device_loop(dev, index, store)
    assert len(got) == len(want) == 3
    blended = 0
    for it, (g, w) in enumerate(zip(got, want)):
        assert g["dil"].dtype == np.int64 and g["dil"].shape == (H, W)
        np.testing.assert_array_equal(g["dil"], w["dil"], err_msg=f"interaction {it}: Dilate_mask")
        assert torch.equal(_bits(g["E"]), _bits(w["E"])), f"interaction {it}: merged estimate"
        assert g["labels"].dtype == np.uint8 and g["labels"].shape == (T, H, W)
        np.testing.assert_array_equal(g["labels"], w["labels"], err_msg=f"interaction {it}: To_np_label")
        np.testing.assert_array_equal(g["labels_u8"].cpu().numpy(), w["labels"], err_msg=f"interaction {it}: the store's labels")
        np.testing.assert_array_equal(g["final_masks"].cpu().numpy(), w["labels"].astype(np.float32))
        assert tuple(g["all_P"].shape) == (T, K, H, W) and torch.equal(_bits(g["all_P"]), _bits(w["all_P"])), f"interaction {it}: all_P"
        blended += int(not torch.equal(w["E"], w["raw"]))
    assert blended == 2 and len(set(np.unique(want[-1]["labels"]).tolist())) == K      # the blend did something; every label occurs
    last = got[-1]
    if index == list(range(K)):                           # the merged estimate IS the store: no copy at all
        assert last["live_all_P"].data_ptr() == last["E"].data_ptr() and store.buf.data_ptr() == last["E"].data_ptr() and store.own is None
    else:                                                 # the store's own buffer, one for the whole session
        assert store.own is not None and last["live_all_P"].data_ptr() == store.own.data_ptr() != last["E"].data_ptr()
        assert got[0]["live_all_P"].data_ptr() == store.own.data_ptr()
    assert last["live_all_P"].stride() == (H * W, T * H * W, W, 1)


def test_label_only_store_feeds_the_assessment_path(dev):
    """probs=False: the same label map and no probability buffer; its LabelMasks is accepted by AssessNet.forward_objects and scores as the
    host loop's label map does."""
    want = host_loop(PERMUTED)
    store = ui.IpnStore(T, K, H, W, dev, probs=False)
    got = device_loop(dev, PERMUTED, store)
    assert store.buf is None and store.own is None
    for g, w in zip(got, want):
        assert isinstance(g["all_P"], LabelMasks) and g["all_P"].map.data_ptr() == store.labels_u8.data_ptr()
        np.testing.assert_array_equal(g["labels_u8"].cpu().numpy(), w["labels"])
        assert torch.equal(_bits(g["E"]), _bits(w["E"]))
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()}, strict=True)
    net.to(dev).eval()
    all_F = torch.rand(T, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    scores = net.forward_objects(all_F, got[-1]["all_P"], O)
    ref = net.forward_objects(all_F, LabelMasks(torch.from_numpy(want[-1]["labels"]).to(dev)), O)
    assert scores.shape == (O, T) and torch.equal(scores.view(torch.int32), ref.view(torch.int32))
    # and it is what the full store's probabilities give once they are made hard
    full = ui.IpnStore(T, K, H, W, dev)
    full_rounds = device_loop(dev, PERMUTED, full)
    assert torch.equal(LabelMasks.from_probs(full_rounds[-1]["live_all_P"]).map, store.labels_u8)
