"""ATNet adapter glue on the hot-path side: ``run_VOS_singleiact`` (reference ``utils/utils_atnet.py:14-161``) with its
torch epilogue replaced by one HIP launch per visited frame (``csrc/atnet_epilogue.hip``) — SURVEY §8(f) row 4, ATNet.

The ATNet network itself (``net.forward_ANet`` / ``net.forward_TNet`` / ``net.encoder_3ch``) is an external clone and stays
whatever the caller passes in, as do the clone's ``libs`` helpers and its DAVIS loader.  What is rebuilt here is everything
between the padded logits and the tensors the rest of the loop consumes: the sigmoid, the blend with the earlier rounds'
probability map (in place), the unblended probabilities the next propagation step takes, and — per frame instead of per
interaction — the labels (``combine_masks_with_batch``) and the cropped probability planes, written once into an
object-major store so that ``assess_all_objects`` reads them in place.  The reference's zero-channel ``torch.cat`` of the
whole probability volume, its strided crop and its float64 host copy of the masks are gone; the labels come to the host as
ONE uint8 copy.  There is no CPU fallback.

The label rule (first maximum over the objects; object + 1 if its probability is strictly above ``th``, else 0) restates
``combine_masks_with_batch`` of the clone's ``libs/utils_torch.py``, which is not part of the reference tree: the rule in
``include/ivosw.h`` is the definition, parity with the clone is unpinned.
"""
import numpy as np
import torch

from .. import _lib as L
from .utils_manet import ProbStore, torch_ptr

SMALLEST_ALPHA = 0.5          # utils/utils_atnet.py:126


class AtnetStore(ProbStore):
    """A ProbStore for an ATNet session: ``buf`` [n_obj + 1, n, H, W] with channel 0 (the reference's ``bg_dummy``) zeroed
    once, ``labels_u8`` [n, H, W] and ``final_masks`` [n, H, W] fp32; ``all_P`` is the permuted [n, n_obj + 1, H, W] view.
    ``probs=False`` makes a label-only store for ``masks=labels`` sessions: no ``buf`` (a 100-frame, 3-object 480p session
    never holds its 656 MB), the kernel gets a NULL probability pointer, and ``all_P`` is the LabelMasks of the label map.
    A slot holds nothing until an epilogue call has written it (``filled``): ``run_VOS_singleiact`` rebuilds every frame it
    has never written from ``prob_map_of_frames`` (the reference's all_P is the crop of the WHOLE map, frames outside the
    propagated range included), so a fresh store on a resumed session comes out complete."""

    def __init__(self, n_frames, n_obj, h, w, device, probs=True):
        if min(int(n_frames), int(n_obj), int(h), int(w)) < 1:
            raise ValueError("AtnetStore: n_frames, n_obj, h and w must be positive")
        self.n_obj = int(n_obj)
        self.buf = None
        if probs:
            self.buf = torch.empty((n_obj + 1, n_frames, h, w), dtype=torch.float32, device=device)
            self.buf[0].zero_()
        self.labels_u8 = torch.zeros((n_frames, h, w), dtype=torch.uint8, device=device)
        self.final_masks = torch.zeros((n_frames, h, w), dtype=torch.float32, device=device)
        self.filled = [False] * int(n_frames)           # frames whose slot and labels an epilogue call has written

    @property
    def all_P(self):
        if self.buf is None:
            from ..models.assessment import LabelMasks
            return LabelMasks(self.labels_u8)
        return self.buf.permute(1, 0, 2, 3)


def prop_alpha(annotated_frames, annotated_now, operating_frame, flag):
    """The weight of the new prediction in the blend with the earlier rounds' map (utils/utils_atnet.py:126-144), in float64
    on the host exactly as there.  flag 1: propagating backward from ``annotated_now``, anything else: forward.  1 when no
    other annotated frame lies in that direction, else 0.5 at that frame rising linearly to 1 at ``annotated_now``."""
    annotated_frames_np = np.array(annotated_frames)
    if flag == 1:
        sorted_frames = annotated_frames_np[annotated_frames_np < annotated_now]
        if len(sorted_frames) == 0:
            return 1
        closest_addianno_frame = np.max(sorted_frames)
        return SMALLEST_ALPHA + (1 - SMALLEST_ALPHA) * (
            (operating_frame - closest_addianno_frame) / (annotated_now - closest_addianno_frame))
    sorted_frames = annotated_frames_np[annotated_frames_np > annotated_now]
    if len(sorted_frames) == 0:
        return 1
    closest_addianno_frame = np.min(sorted_frames)
    return SMALLEST_ALPHA + (1 - SMALLEST_ALPHA) * (
        (closest_addianno_frame - operating_frame) / (closest_addianno_frame - annotated_now))


def check_pads(pads):
    hpad1, hpad2, wpad1, wpad2 = (int(v) for v in pads)
    if hpad1 < 0 or wpad1 < 0 or hpad2 < 0 or wpad2 < 0:
        raise ValueError(f"atnet_epilogue: negative pad in {tuple(pads)}")
    if hpad2 == 0 or wpad2 == 0:
        raise ValueError(f"atnet_epilogue: hpad2 and wpad2 must be positive, got {tuple(pads)}: the reference crops with "
                         "[hpad1:-hpad2, wpad1:-wpad2], which is EMPTY for a zero trailing pad")
    return hpad1, hpad2, wpad1, wpad2


def atnet_epilogue(logits, prob_map_of_frames, frame, pads, th, store, alpha=None):
    """One kernel call for frame ``frame``.

    logits [n_obj, 1, PH, PW] (or [n_obj, PH, PW]) fp32 on the device, or None: rebuild the frame's labels and store slot
    from ``prob_map_of_frames[frame]`` as it stands (nothing blended, the map not written).  prob_map_of_frames
    [n, n_obj, PH, PW] fp32 contiguous on the device, updated in place.  pads = (hpad1, hpad2, wpad1, wpad2).
    alpha=None: the interaction frame (no blend); otherwise the blend weight of ``prop_alpha``.
    Returns prob_pad [n_obj, 1, PH, PW], the unblended sigmoid (None without logits)."""
    pm = prob_map_of_frames
    if not isinstance(pm, torch.Tensor) or pm.dim() != 4 or pm.dtype != torch.float32 or not pm.is_contiguous():
        raise ValueError("atnet_epilogue: prob_map_of_frames must be a contiguous float32 [n, n_obj, PH, PW] (it is updated in place)")
    hpad1, hpad2, wpad1, wpad2 = check_pads(pads)
    n, n_obj, PH, PW = (int(v) for v in pm.shape)
    h, w = (int(v) for v in store.labels_u8.shape[1:])
    frame = int(frame)
    if not 0 <= frame < n:
        raise ValueError(f"atnet_epilogue: frame {frame} outside [0, {n})")
    if PH != hpad1 + h + hpad2 or PW != wpad1 + w + wpad2:
        raise ValueError(f"atnet_epilogue: padded grid {PH}x{PW} is not the store's {h}x{w} plus the pads {tuple(pads)}")
    if store.labels_u8.shape[0] != n or store.final_masks.shape != store.labels_u8.shape or store.labels_u8.device != pm.device:
        raise ValueError("atnet_epilogue: the store does not match prob_map_of_frames")
    if store.buf is not None and tuple(store.buf.shape) != (n_obj + 1, n, h, w):
        raise ValueError("atnet_epilogue: the store's probability buffer does not match prob_map_of_frames")
    if alpha is not None and logits is None:
        raise ValueError("atnet_epilogue: a blend needs logits")
    dev = pm.device
    x = prob_pad = None
    if logits is not None:
        if not isinstance(logits, torch.Tensor) or tuple(logits.shape) not in ((n_obj, 1, PH, PW), (n_obj, PH, PW)):
            raise ValueError(f"atnet_epilogue: logits are not [{n_obj}, 1, {PH}, {PW}]")
        if not (logits.is_cuda and pm.is_cuda):
            raise RuntimeError("atnet_epilogue: logits and prob_map_of_frames must be CUDA tensors (no CPU fallback)")
        x = logits.detach()
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        prob_pad = torch.empty((n_obj, 1, PH, PW), dtype=torch.float32, device=dev)
    blend = alpha is not None
    alpha32 = float(np.float32(alpha)) if blend else 1.0
    beta32 = float(np.float32(1 - np.float64(alpha))) if blend else 0.0          # 1 - alpha in float64, then rounded: torch's scalar
    hw = h * w
    L.check(L.lib().ivosw_atnet_epilogue(
        L.dptr(x) if x is not None else None, torch_ptr(pm, frame * n_obj * PH * PW), n_obj, PH, PW, hpad1, wpad1, h, w,
        int(blend), alpha32, beta32, float(np.float32(th)), L.dptr(prob_pad) if prob_pad is not None else None,
        torch_ptr(store.buf, (n + frame) * hw) if store.buf is not None else None, n * hw,
        torch_ptr(store.labels_u8, frame * hw), torch_ptr(store.final_masks, frame * hw), L.stream_ptr(dev)), "atnet_epilogue")
    store.filled[frame] = True
    return prob_pad


def run_VOS_singleiact(net, config, split, scribbles_data, annotated_frames, final_masks, num_frames, n_objects, n_interaction, subseq,
                       pad_info, anno_3chEnc_r5_list, anno_6chEnc_r5_list, prob_map_of_frames, hpad1, hpad2, wpad1, wpad2,
                       loader=None, libs=None, store=None):
    """Same signature and return value as the reference's ``run_VOS_singleiact`` (``output_masks`` numpy float64 [n, H, W],
    ``all_P`` [n, O+1, H, W] fp32 on the device — the store's view) plus three optional keywords: ``loader`` (an iterable of
    the reference's batched dicts, in place of the DAVIS2017 + DataLoader built otherwise), ``libs`` (the clone's ``utils``
    helpers ``get_prop_list`` and ``scribble_to_image``; default: ``from libs import utils`` as the reference does) and
    ``store`` (an AtnetStore to reuse across interactions; a label-only one returns a LabelMasks in all_P's place).
    Control flow follows utils/utils_atnet.py:14-161 line by line; ``prob_map_of_frames`` is updated in place."""
    pads = check_pads((hpad1, hpad2, wpad1, wpad2))
    if libs is None:
        from libs import utils as libs               # the ATNet clone's helpers, as in the reference
    dev = prob_map_of_frames.device
    th = config.test_propth
    annotated_now = annotated_frames[-1]
    scribbles_list = scribbles_data['scribbles']
    seq_name = scribbles_data['sequence']

    output_masks = final_masks.copy().astype(np.float64)
    if store is None:
        store = AtnetStore(num_frames, n_objects, output_masks.shape[1], output_masks.shape[2], dev)

    prop_list = libs.get_prop_list(annotated_frames, annotated_now, num_frames, proportion=config.test_propagation_proportion)
    prop_fore = sorted(prop_list)[0]
    prop_rear = sorted(prop_list)[-1]

    # Interaction settings
    pm_ps_ns_3ch_t = []  # n_obj,3,h,w
    if n_interaction == 1:
        for obj_id in range(1, n_objects + 1):
            pos_scrimg = libs.scribble_to_image(scribbles_list, annotated_now, obj_id, dilation=config.scribble_dilation_param,
                                                prev_mask=final_masks[annotated_now])
            pm_ps_ns_3ch_t.append(np.stack([np.ones_like(pos_scrimg) / 2, pos_scrimg, np.zeros_like(pos_scrimg)], axis=0))
    else:
        for obj_id in range(1, n_objects + 1):
            prev_round_input = (final_masks[annotated_now] == obj_id).astype(np.float32)  # H,W
            pos_scrimg, neg_scrimg = libs.scribble_to_image(scribbles_list, annotated_now, obj_id, dilation=config.scribble_dilation_param,
                                                            prev_mask=final_masks[annotated_now], blur=True, singleimg=False,
                                                            seperate_pos_neg=True)
            pm_ps_ns_3ch_t.append(np.stack([prev_round_input, pos_scrimg, neg_scrimg], axis=0))
    pm_ps_ns_3ch_t = torch.from_numpy(np.stack(pm_ps_ns_3ch_t, axis=0)).to(dev)  # n_obj,3,h,w

    if (prop_list[0] != annotated_now) and (prop_list.count(annotated_now) != 2):
        raise NotImplementedError
    # the prop list goes backward first, then forward

    if loader is None:
        from torch.utils.data import DataLoader
        from torchvision import transforms
        from datasets.davis_dataset import DAVIS2017           # the ATNet clone's dataset, as in the reference
        from libs import custom_transforms as tr
        composed_transforms = transforms.Compose([tr.Normalize_ApplymeanvarImage(config.mean, config.var), tr.ToTensor()])
        db_test = DAVIS2017(split=split, subseq=subseq, transform=composed_transforms, root=config.davis_dataset_dir,
                            custom_frames=prop_list, seq_name=seq_name, rgb=True, obj_id=None, no_gt=True, retname=True,
                            prev_round_masks=final_masks)
        loader = DataLoader(db_test, batch_size=1, shuffle=False, num_workers=4, pin_memory=True)

    flag = 0  # 1: propagating backward, 2: propagating forward
    visited = set()
    for ii, batched in enumerate(loader):
        # batched : image, scr_img, 0~fr, meta
        inpdict = dict()
        operating_frame = int(batched['meta']['frame_id'][0])
        for inp in batched:
            if inp == 'meta':
                continue
            inpdict[inp] = batched[inp].to(dev)
        inpdict['image'] = inpdict['image'].expand(n_objects, -1, -1, -1)

        #################### Iaction ########################
        if operating_frame == annotated_now:  # Check the round is on interaction
            if flag == 0:
                flag += 1
                adjacent_to_anno = True
            elif flag == 1:
                flag += 1
                adjacent_to_anno = True
                continue
            else:
                raise NotImplementedError

            pm_ps_ns_3ch_t = torch.nn.ReflectionPad2d(pad_info[1] + pad_info[0])(pm_ps_ns_3ch_t)
            inputs = torch.cat([inpdict['image'], pm_ps_ns_3ch_t], dim=1)
            output_logit, anno_6chEnc_r5 = net.forward_ANet(inputs)  # [nobj, 1, P_H, P_W], # [n_obj,2048,h/16,w/16]
            output_prob_anno = atnet_epilogue(output_logit, prob_map_of_frames, operating_frame, pads, th, store)

            anno_3chEnc_r5, _, _, r2_prev_fromanno = net.encoder_3ch.forward(inpdict['image'])
            anno_6chEnc_r5_list.append(anno_6chEnc_r5)
            anno_3chEnc_r5_list.append(anno_3chEnc_r5)

            if len(anno_6chEnc_r5_list) != len(annotated_frames):
                raise NotImplementedError

        #################### Propagation ########################
        else:
            # Flag [1: propagating backward, 2: propagating forward]
            if adjacent_to_anno:
                r2_prev = r2_prev_fromanno
                predmask_prev = output_prob_anno
            else:
                predmask_prev = output_prob_prop
            adjacent_to_anno = False

            output_logit, r2_prev = net.forward_TNet(anno_3chEnc_r5_list, inpdict['image'], anno_6chEnc_r5_list,
                                                     r2_prev, predmask_prev)  # [nobj, 1, P_H, P_W]
            alpha = prop_alpha(annotated_frames, annotated_now, operating_frame, flag)
            output_prob_prop = atnet_epilogue(output_logit, prob_map_of_frames, operating_frame, pads, th, store, alpha=alpha)
        visited.add(operating_frame)

    # labels and slot from the map as it is: a frame of the range the loop did not visit, and any frame the store has never held
    for t in range(num_frames):
        if t not in visited and (prop_fore <= t <= prop_rear or not store.filled[t]):
            atnet_epilogue(None, prob_map_of_frames, t, pads, th, store)

    output_masks[prop_fore:prop_rear + 1] = store.labels_u8[prop_fore:prop_rear + 1].cpu().numpy().astype(np.float64)  # f,h,w
    return output_masks, store.all_P
