"""Seed / meter / checkpoint helpers with the reference's names and behaviour (utils/misc.py:11-115).

``sequence_metric`` (:118-162) keeps the reference's signature; its J / F measures run on the device
(``ivos_w_amd.metrics`` -> ``ivosw_jf_counts``) instead of the third-party ``davisinteractive`` package.
"""
import os
import random
from collections import OrderedDict

import numpy as np
import torch


def set_random_seed(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class AverageMeter:
    """Running average (val, sum, count, avg)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _strip_module(k):
    return k[7:] if "module" in k else k


def save_network_checkpoint(ckpt_dir, assess_net):
    """Writes ``assess_net.pt`` = the state_dict as-is (the reference builds a stripped CPU copy but saves the
    original dict, utils/misc.py:42-49; the file content is therefore the plain state_dict)."""
    os.makedirs(ckpt_dir, exist_ok=True)
    torch.save(assess_net.state_dict(), os.path.join(ckpt_dir, "assess_net.pt"))


def load_network_checkpoint(ckpt_path, encoder=None, device="cpu", strict=True):
    """Returns False when the file is missing; strips 'module.' for device='cpu', adds it for device='gpu'."""
    if not os.path.exists(ckpt_path):
        return False
    sd = torch.load(ckpt_path, map_location="cpu")
    fixed = OrderedDict()
    for k, v in sd.items():
        if device == "cpu" and "module" in k:
            k = k[7:]
        elif device == "gpu" and "module" not in k:
            k = "module." + k
        fixed[k] = v
    encoder.load_state_dict(fixed, strict=strict)
    return True


def save_agent_checkpoint(net, ckpt_dir, epoch=None):
    os.makedirs(ckpt_dir, exist_ok=True)
    name = "agent.pt" if epoch is None else f"agent_epoch_{epoch}.pt"
    torch.save(OrderedDict((k, v.detach().clone().to("cpu")) for k, v in net.state_dict().items()),
               os.path.join(ckpt_dir, name))


def load_agent_checkpoint(agent, ckpt_dir, device="cpu", strict=False):
    """Never raises (utils/misc.py:99-115): returns None when agent/file is missing, 1 on success, -1 on failure."""
    if agent is None:
        return
    path = os.path.join(ckpt_dir, "agent.pt")
    if not os.path.exists(path):
        print(f"no model found in {path}")
        return
    print(f"load agent model from {path}")
    try:
        sd = torch.load(path, map_location="cpu")
        fixed = OrderedDict()
        for k, v in sd.items():
            k = _strip_module(k)
            if "base" in k and "encoder" not in k:
                k = "encoder." + k
            if str(device) == "cuda":
                k = "module." + k
            fixed[k] = v
        agent.policy_net.load_state_dict(fixed, strict=strict)
        return 1
    except Exception:
        print(f"catch some EXCEPTION when trying to load {path}")
        return -1


def sequence_metric(metric_to_optimize, gt_masks, pred_masks, nb_objects, average_over_objects=True,
                    convert_to_single_obj=False):
    """utils/misc.py:118-162 with the davisinteractive metrics computed on the device (ivos_w_amd.metrics).

    gt_masks / pred_masks: [N,H,W] integer label maps, numpy arrays (as the reference's callers pass them) or tensors
    (device tensors avoid the upload).  Returns the numpy float64 array the reference returns.  Like the reference,
    ``convert_to_single_obj`` rewrites the caller's arrays in place."""
    from .. import metrics

    if convert_to_single_obj:
        gt_masks[gt_masks > 0] = 1
        pred_masks[pred_masks > 0] = 1
        nb_objects = 1

    if metric_to_optimize == 'J':
        metric = metrics.batched_jaccard(gt_masks, pred_masks, average_over_objects=average_over_objects,
                                         nb_objects=nb_objects)
    elif metric_to_optimize == 'F':
        metric = metrics.batched_f_measure(gt_masks, pred_masks, average_over_objects=average_over_objects,
                                           nb_objects=nb_objects)
    elif metric_to_optimize == 'J_AND_F':
        jaccard, contour = metrics.batched_j_and_f(gt_masks, pred_masks, average_over_objects=average_over_objects,
                                                   nb_objects=nb_objects)
        metric = .5 * jaccard + .5 * contour
    return metric


def sequence_metric_videos(metric_to_optimize, videos, average_over_objects=True):
    """``sequence_metric`` for several videos at once: ``videos`` = [(gt_masks, pred_masks, nb_objects), ...], each of its own length and
    size.  One J / F pass on the device for all of them, the float64 ratios and the mean over the objects included
    (``metrics.jf_videos``), and ONE device-to-host copy.  Returns one numpy float64 array per video - [N], or [N,O] without the average -
    equal to ``sequence_metric`` on that video, bit for bit."""
    from .. import metrics

    res = metrics.jf_videos(videos, metric_to_optimize, per_object=not average_over_objects)
    if average_over_objects:
        host = res.quality.cpu().numpy()                                 # the one D2H copy of the call
        offs = np.concatenate([[0], np.cumsum(res.lengths)])
        return [host[int(a):int(b)].copy() for a, b in zip(offs[:-1], offs[1:])]
    host = res.per_object_flat.cpu().numpy()
    offs = np.concatenate([[0], np.cumsum([n * o for n, o in zip(res.lengths, res.n_obj)])])
    return [host[int(a):int(b)].reshape(n, o).copy() for a, b, n, o in zip(offs[:-1], offs[1:], res.lengths, res.n_obj)]


def write_gray(path_stem, plane):
    """A uint8 [H,W] plane to ``path_stem`` + ".png" (8-bit greyscale) through PIL when it is importable, else + ".pgm" (binary P5) from
    plain Python.  Returns the path written."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    try:
        from PIL import Image
    except ImportError:
        path = path_stem + ".pgm"
        with open(path, "wb") as fp:
            fp.write(b"P5\n%d %d\n255\n" % (plane.shape[1], plane.shape[0]) + plane.tobytes())
        return path
    path = path_stem + ".png"
    Image.fromarray(plane, mode="L").save(path)
    return path


def save_seg_preds(probs, new_masks_meta, save_result_dir):
    """utils/misc.py:165-181 with the bytes formed on the device: the reference copies the whole float32 all_P to the host and writes
    ``probs[i, n] * 255`` per object plane through cv2.imwrite; here ONE ``metrics.quantize_probs`` launch forms the same bytes where
    all_P lives and ONE uint8 copy - a quarter of the bytes - reaches the host.  Same signature and directory layout:
    <save_result_dir>/interaction-{n}/scribble-{s}/{sequence}/probs/{obj}/{i:05d}.png for the objects 1 .. O (channel 0 is not written),
    8-bit greyscale through PIL (binary .pgm without it).  ``probs``: all_P as ``quantize_probs`` takes it ([n, O+1, H, W] float32 on the
    device, a store, or a host array), or the already quantised uint8 [O, n, H, W] device tensor.  Returns the paths written, object-major."""
    from .. import metrics

    if isinstance(probs, torch.Tensor) and probs.dtype == torch.uint8:
        if probs.ndim != 4:
            raise ValueError(f"save_seg_preds: quantised planes must be uint8 [O, n, H, W], got {tuple(probs.shape)}")
        planes = probs
    else:
        p = probs.all_P if hasattr(probs, "all_P") else probs
        planes = metrics.quantize_probs(p, int(p.shape[1]) - 1)
    host = planes.cpu().numpy()                                          # the one D2H copy of the call
    meta = new_masks_meta
    root = os.path.join(save_result_dir, f"interaction-{meta['n_interaction']}", f"scribble-{meta['scribble_iter']}", meta["sequence"], "probs")
    paths = []
    for o in range(host.shape[0]):                                       # object o + 1; channel 0 has no directory
        obj_dir = os.path.join(root, str(o + 1))
        os.makedirs(obj_dir, exist_ok=True)
        paths += [write_gray(os.path.join(obj_dir, f"{i:05d}"), host[o, i]) for i in range(host.shape[1])]
    return paths
