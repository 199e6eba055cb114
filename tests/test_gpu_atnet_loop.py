"""GPU: utils_atnet.run_VOS_singleiact driven with doubles - a 7-frame, 2-object, 16 x 28 video padded to 20 x 36, two interactions
(frame 1, then frame 5, each propagated 3 frames either way) - against the same loop written with torch ops, on the device, in float32,
and against that loop in float64.

The net double returns seeded logits of the right shapes (they do not depend on what it is handed, so all three loops see the same
logits) and records the predmask_prev it was handed; the libs double has a contiguous get_prop_list; the loader is a list.

Probabilities: the kernel loop's largest error against the float64 loop is held to SIG_MULT * (the float32 torch loop's error against
the same float64 values) + 2^-24, the bar of tests/test_gpu_atnet_epilogue.py (LAB_NOTES.md, "ATNet epilogue against float64").
Labels: equal to the float64 loop's wherever the decision is safe - the float64 top-two gap and the gap of the best to th both exceed
MARGIN = 2 * (E + 4 * 2^-24), E that bar evaluated: either contestant may be off by E, and the blend adds at most four float32
roundings of values <= 1 (alpha, 1 - alpha, two products and a sum make five, of which the sum's operands are already counted once).
At most 1e-3 of the pixels may be unsafe - a cap, not a tolerance; the torch loop alone is held to the same.
"""
import types

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import synth
from ivos_w_amd.models.assessment import AssessNet, LabelMasks
from ivos_w_amd.utils import utils_atnet as ua
from tests.atnet_ref import SIG_MULT

pytestmark = pytest.mark.gpu

N, O, H, W = 7, 2, 16, 28
PADS = (2, 2, 4, 4)                                       # hpad1, hpad2, wpad1, wpad2
PH, PW = H + PADS[0] + PADS[1], W + PADS[2] + PADS[3]
TH = 0.6
ANNOTATED = (1, 5)
CONFIG = types.SimpleNamespace(test_propth=TH, test_propagation_proportion=3 / 7, scribble_dilation_param=5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


class Libs:
    """The clone's libs.utils, as far as run_VOS_singleiact uses it."""

    @staticmethod
    def get_prop_list(annotated_frames, annotated_now, num_frames, proportion=1.0):
        r = int(round(proportion * num_frames))
        back = list(range(annotated_now, max(annotated_now - r, 0) - 1, -1))
        return back + list(range(annotated_now, min(annotated_now + r, num_frames - 1) + 1))

    @staticmethod
    def scribble_to_image(scribbles, frame, obj_id, dilation=0, prev_mask=None, blur=False, singleimg=True, seperate_pos_neg=False):
        img = np.zeros(prev_mask.shape, np.float32)
        img[2 + obj_id:6 + obj_id, 3:9] = 1.0
        return (img, img[::-1].copy()) if seperate_pos_neg else img


class Net:
    """Seeded logits, one draw per call: two Nets made with the same seed answer the same sequence of calls with the same logits."""

    def __init__(self, dev, dtype=torch.float32):
        self.g = torch.Generator().manual_seed(2024)
        self.dev, self.dtype = dev, dtype
        self.prev = []                                    # what forward_TNet was handed as predmask_prev
        self.logits = []
        self.encoder_3ch = types.SimpleNamespace(forward=self._encode)

    def _logit(self):
        x = (torch.randn(O, 1, PH, PW, generator=self.g) * 3).to(self.dev)
        self.logits.append(x)
        return x.to(self.dtype)

    def _encode(self, image):
        assert tuple(image.shape) == (O, 3, PH, PW)
        return torch.zeros(O, 4, 2, 2, device=self.dev), None, None, torch.zeros(O, 2, 5, 9, device=self.dev)

    def forward_ANet(self, inputs):
        assert tuple(inputs.shape) == (O, 6, PH, PW)
        return self._logit(), torch.zeros(O, 8, 2, 2, device=self.dev)

    def forward_TNet(self, a3, image, a6, r2_prev, predmask_prev):
        assert len(a3) == len(a6) and tuple(predmask_prev.shape) == (O, 1, PH, PW)
        self.prev.append(predmask_prev)
        return self._logit(), r2_prev


def _loader(annotated, now):
    g = torch.Generator().manual_seed(7)
    frames = torch.rand(N, 3, PH, PW, generator=g)
    return [{"image": frames[t:t + 1], "meta": {"frame_id": [t]}} for t in Libs.get_prop_list(annotated, now, N, CONFIG.test_propagation_proportion)]


def _initial(dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(11)
    pm = torch.rand(N, O, PH, PW, generator=g).to(dev).to(dtype)
    fm = np.random.default_rng(3).integers(0, O + 1, (N, H, W)).astype(np.float64)
    return pm, fm


def _session(dev, run, dtype=torch.float32, **kw):
    """Two interactions through `run` (run_VOS_singleiact or its torch restatement); returns what the second one returned and the state."""
    pm, fm = _initial(dev, dtype)
    net = Net(dev, dtype)
    a3, a6 = [], []
    res = []
    for k, now in enumerate(ANNOTATED):
        annotated = list(ANNOTATED[:k + 1])
        masks, all_P = run(net, CONFIG, "val", {"scribbles": [], "sequence": "seq"}, annotated, fm, N, O, k + 1, None, (PADS[:2], PADS[2:]), a3, a6,
                           pm, *PADS, loader=_loader(annotated, now), libs=Libs, **kw)
        res.append((masks, all_P if not isinstance(all_P, torch.Tensor) else all_P.clone()))
        fm = masks
    return res, pm, net


def torch_loop(net, config, split, scribbles_data, annotated_frames, final_masks, num_frames, n_objects, n_interaction, subseq, pad_info,
               anno_3chEnc_r5_list, anno_6chEnc_r5_list, prob_map_of_frames, hpad1, hpad2, wpad1, wpad2, loader=None, libs=None):
    """The reference's loop with its torch ops (utils/utils_atnet.py:72-159), in the dtype of the map; combine_masks_with_batch by the
    rule of include/ivosw.h."""
    annotated_now = annotated_frames[-1]
    output_masks = final_masks.copy().astype(np.float64)
    prop_list = libs.get_prop_list(annotated_frames, annotated_now, num_frames, proportion=config.test_propagation_proportion)
    prop_fore, prop_rear = sorted(prop_list)[0], sorted(prop_list)[-1]
    flag = 0
    for batched in loader:
        operating_frame = int(batched['meta']['frame_id'][0])
        image = batched['image'].to(prob_map_of_frames.device).expand(n_objects, -1, -1, -1)
        if operating_frame == annotated_now:
            if flag == 0:
                flag += 1
                adjacent_to_anno = True
            else:
                flag += 1
                adjacent_to_anno = True
                continue
            output_logit, e6 = net.forward_ANet(torch.cat([image, image], 1))
            output_prob_anno = torch.sigmoid(output_logit)
            prob_onehot_t = output_prob_anno[:, 0].detach()
            e3, _, _, r2_prev_fromanno = net.encoder_3ch.forward(image)
            anno_6chEnc_r5_list.append(e6)
            anno_3chEnc_r5_list.append(e3)
        else:
            if adjacent_to_anno:
                r2_prev = r2_prev_fromanno
                predmask_prev = output_prob_anno
            else:
                predmask_prev = output_prob_prop
            adjacent_to_anno = False
            output_logit, r2_prev = net.forward_TNet(anno_3chEnc_r5_list, image, anno_6chEnc_r5_list, r2_prev, predmask_prev)
            output_prob_prop = torch.sigmoid(output_logit)
            prob_onehot_t = output_prob_prop[:, 0].detach()
            alpha = ua.prop_alpha(annotated_frames, annotated_now, operating_frame, flag)
            prob_onehot_t = (alpha * prob_onehot_t) + ((1 - alpha) * prob_map_of_frames[operating_frame])
        prob_map_of_frames[operating_frame] = prob_onehot_t
    p = prob_map_of_frames[prop_fore:prop_rear + 1]
    am = p.argmax(1, keepdim=True)                        # the first maximum
    lab = torch.where(p.gather(1, am) > config.test_propth, am + 1, torch.zeros_like(am))
    output_masks[prop_fore:prop_rear + 1] = lab[:, 0, hpad1:-hpad2, wpad1:-wpad2].cpu().numpy().astype(np.float64)
    bg_dummy = torch.zeros_like(prob_map_of_frames[:, 0:1])
    return output_masks, torch.cat([bg_dummy, prob_map_of_frames], 1)[:, :, hpad1:-hpad2, wpad1:-wpad2]


@pytest.fixture(scope="module")
def loops(dev):
    """The three loops, run once: (results, final map, net) of the kernel loop with its store, of the float32 torch loop and of the
    float64 torch loop."""
    store = ua.AtnetStore(N, O, H, W, dev)
    return {"kernel": _session(dev, ua.run_VOS_singleiact, store=store) + (store,), "torch": _session(dev, torch_loop),
            "f64": _session(dev, torch_loop, torch.float64)}


def test_two_interactions_against_the_torch_loop(dev, loops):
    (res_k, pm_k, net_k, store), (res_t, pm_t, _), (res_d, pm_d, _) = loops["kernel"], loops["torch"], loops["f64"]
    pm0, fm0 = _initial(dev)
    for k in range(2):
        P_k, P_t, P_d = (r[k][1].double() for r in (res_k, res_t, res_d))
        assert tuple(res_k[k][1].shape) == (N, O + 1, H, W) and res_k[k][1].dtype == torch.float32 and (P_k[:, 0] == 0).all()
        err_k, err_t = float((P_k - P_d).abs().max()), float((P_t - P_d).abs().max())
        print(f"ATNETLOOP interaction {k + 1} err_kernel={err_k:.3e} err_torch={err_t:.3e}")
        E = SIG_MULT * err_t + 2.0 ** -24
        assert err_k <= E, (err_k, err_t)
        # labels wherever the float64 decision is safe
        margin = 2 * (E + 4 * 2.0 ** -24)
        top = P_d[:, 1:].topk(2, dim=1).values if O > 1 else None
        safe = ((top[:, 0] - top[:, 1]) > margin) & ((top[:, 0] - TH).abs() > margin)
        unsafe = float((~safe).double().mean())
        print(f"ATNETLOOP interaction {k + 1} unsafe pixels {unsafe:.2e}")
        assert unsafe <= 1e-3
        safe = safe.cpu().numpy()
        m_k, m_t, m_d = res_k[k][0], res_t[k][0], res_d[k][0]
        assert m_k.dtype == np.float64 and m_k.shape == (N, H, W)
        assert (m_k[safe] == m_d[safe]).all() and (m_t[safe] == m_d[safe]).all()
        # frames outside the propagated range keep final_masks
        lo, hi = max(ANNOTATED[k] - 3, 0), min(ANNOTATED[k] + 3, N - 1)
        before = fm0 if k == 0 else res_k[0][0]
        outside = [t for t in range(N) if not lo <= t <= hi]
        assert outside and (m_k[outside] == before[outside]).all()
    # the store holds the last interaction's labels, and the returned all_P is its view
    np.testing.assert_array_equal(store.labels_u8[2:].cpu().numpy(), res_k[1][0][2:].astype(np.uint8))
    np.testing.assert_array_equal(store.final_masks[2:].cpu().numpy(), res_k[1][0][2:].astype(np.float32))
    assert torch.equal(store.all_P, res_k[1][1]) and store.all_P.data_ptr() == store.buf.data_ptr()
    # the map is mutated in place (every frame was propagated in one of the two interactions), its padded border included
    assert not torch.equal(pm_k, pm0) and float((pm_k.double() - pm_d).abs().max()) <= SIG_MULT * float((pm_t.double() - pm_d).abs().max()) + 2.0 ** -24
    assert torch.equal(ua_crop(pm_k), store.all_P[:, 1:])


def ua_crop(pm):
    return pm[:, :, PADS[0]:PH - PADS[1], PADS[2]:PW - PADS[3]]


def test_frames_outside_the_range_are_untouched_and_launches_are_counted(dev, monkeypatch):
    """One interaction on frame 1 (range 0 .. 4): frames 5 and 6 of the map, of the store and of the masks keep their bits; exactly one
    epilogue launch per visited frame; each predmask_prev handed to the net is the prob_pad the previous epilogue call returned."""
    real = L.lib()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "ivosw_atnet_epilogue":
                return fn

            def counted(*a):
                calls.append(a)
                return fn(*a)
            return counted

    returned = []
    real_epilogue = ua.atnet_epilogue

    def recording(*a, **kw):
        returned.append(real_epilogue(*a, **kw))
        return returned[-1]

    monkeypatch.setattr(L, "lib", lambda: Counting())
    monkeypatch.setattr(ua, "atnet_epilogue", recording)
    pm, fm = _initial(dev)
    pm0 = pm.clone()
    net = Net(dev)
    store = ua.AtnetStore(N, O, H, W, dev)
    store.buf[1:].fill_(-7.0)
    ptr = pm.data_ptr()
    masks, all_P = ua.run_VOS_singleiact(net, CONFIG, "val", {"scribbles": [], "sequence": "seq"}, [1], fm, N, O, 1, None, (PADS[:2], PADS[2:]), [], [],
                                         pm, *PADS, loader=_loader([1], 1), libs=Libs, store=store)
    torch.cuda.synchronize(dev)
    visited = [1, 0, 2, 3, 4]                             # the second visit of frame 1 is skipped
    with_logits = [a for a in calls if a[0] is not None]
    assert len(with_logits) == len(visited) == len(net.logits) and len(returned) == len(calls) == len(visited) + 2
    returned = [r for r in returned if r is not None]
    # frames 5 and 6: the map keeps its bits; the fresh store takes their slots and labels from the map as it stands (one logits = NULL
    # call each - the reference's all_P is the crop of the whole map); the masks returned keep final_masks there
    assert pm.data_ptr() == ptr and torch.equal(pm[5:], pm0[5:]) and not torch.equal(pm[:5], pm0[:5])
    assert torch.equal(store.all_P[5:, 1:], ua_crop(pm0)[5:]) and (store.buf[0] == 0).all() and all(store.filled)
    best, am = ua_crop(pm0)[5:].max(1)
    assert torch.equal(store.labels_u8[5:].long(), torch.where(best > float(np.float32(TH)), ua_crop(pm0)[5:].argmax(1) + 1, 0))
    assert torch.equal(store.final_masks[5:], store.labels_u8[5:].float())
    assert (masks[5:] == fm[5:]).all() and set(np.unique(masks[:5]).tolist()) <= {0.0, 1.0, 2.0}
    # predmask_prev: the annotated frame's prob_pad for the first step of either direction, else the previous step's - the very tensors
    want = [returned[0], returned[0], returned[2], returned[3]]
    assert len(net.prev) == 4 and all(a is b for a, b in zip(net.prev, want))
    for x, s in zip(net.logits, returned):                # and each is the sigmoid of that call's logits (alpha = 1: also the map's frame)
        assert tuple(s.shape) == (O, 1, PH, PW) and float((s - torch.sigmoid(x)).abs().max()) <= (SIG_MULT + 1) * 2.0 ** -24
    for t, s in zip(visited, returned):
        assert torch.equal(pm[t], s[:, 0])
    # a second interaction on the same store: every frame has been written, so one launch per visited frame and nothing else
    del calls[:]
    ua.run_VOS_singleiact(net, CONFIG, "val", {"scribbles": [], "sequence": "seq"}, [1, 5], masks, N, O, 2, None, (PADS[:2], PADS[2:]), [0], [0],
                          pm, *PADS, loader=_loader([1, 5], 5), libs=Libs, store=store)
    assert len(calls) == 5 and all(a[0] is not None for a in calls)


def test_label_only_store(dev, loops):
    """probs=False: the same label map, no probability buffer, and the scores of the label path.  LabelMasks.from_probs(all_P) is the
    argmax over [0, p_1 .. p_O] - the label rule at th = 0 - so a session run at th = 0 is compared with it; the session at TH is compared
    with the full store's own label map."""
    res_k, _, _, full = loops["kernel"]
    store = ua.AtnetStore(N, O, H, W, dev, probs=False)
    res_l, _, _ = _session(dev, ua.run_VOS_singleiact, store=store)
    assert store.buf is None and isinstance(res_l[1][1], LabelMasks) and res_l[1][1].map.data_ptr() == store.labels_u8.data_ptr()
    assert torch.equal(store.labels_u8, full.labels_u8) and torch.equal(store.final_masks, full.final_masks)
    for k in range(2):
        np.testing.assert_array_equal(res_l[k][0], res_k[k][0])
    net = AssessNet(precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()}, strict=True)
    net.to(dev).eval()
    all_F = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    got = net.forward_objects(all_F, res_l[1][1], O)
    want = net.forward_objects(all_F, LabelMasks(full.labels_u8), O)
    assert got.shape == (O, N) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # th = 0: the label rule IS from_probs' argmax
    zero = types.SimpleNamespace(**{**vars(CONFIG), "test_propth": 0.0})
    full0, lab0 = ua.AtnetStore(N, O, H, W, dev), ua.AtnetStore(N, O, H, W, dev, probs=False)
    for st in (full0, lab0):
        pm, fm = _initial(dev)
        ua.run_VOS_singleiact(Net(dev), zero, "val", {"scribbles": [], "sequence": "seq"}, [1], fm, N, O, 1, None, (PADS[:2], PADS[2:]), [], [],
                              pm, *PADS, loader=_loader([1], 1), libs=Libs, store=st)
    from_probs = LabelMasks.from_probs(full0.all_P[:5])
    assert torch.equal(from_probs.map, lab0.labels_u8[:5])
    got = net.forward_objects(all_F[:5], LabelMasks(lab0.labels_u8[:5]), O)
    want = net.forward_objects(all_F[:5], from_probs, O)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
