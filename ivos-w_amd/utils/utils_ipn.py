"""IPN adapter glue on the hot-path side: the host code of the reference's ``utils/utils_ipn.py`` between the IPN network and the
tensors the rest of the loop consumes, on the device (``csrc/ipn_glue.hip``) — SURVEY §8(f) row 4, IPN.

The IPN network itself (``model.Run``) is an external clone and stays whatever the caller passes in.  What is rebuilt here:

* ``Dilate_mask`` (:26-34): the reference makes one cv2 dilation call per object on the CPU; here ONE launch of ``ivosw_ipn_dilate``
  covers every object and, through ``dilate_scribbles``, every scribble map of a batch.  The kernel's rule (the largest object found in
  the radius-2 diamond, -1 if none) is what the reference's loop yields: two iterations of the 3x3 cross are that diamond, cv2's
  default border never contributes to a dilation, and the ascending object loop with overwrite is a maximum.  This was checked against
  ``scipy.ndimage.binary_dilation`` per object (tests/ipn_ref.py); cv2 is not a dependency of this package, so parity with cv2 itself
  is restated, not recorded.
* the round merge with the ``Get_weight`` weights (:37-72), ``To_np_label`` (:75-81) and ``all_P`` (eval_agent_ipn.py:261):
  ``merge_round`` is ONE ``ivosw_ipn_merge`` call for the whole session.  IPN's estimate is already object-major, the layout
  ``ProbStore`` was built around: with an identity channel order the merged estimate IS the store and ``all_P`` is a view of it, with
  no copy at all.  The labels come to the host as ONE uint8 copy instead of the whole float estimate.

The blend rule (``w * new + (1 - w) * old``, three separately rounded fp32 operations on every frame) is this project's definition:
IPN's ``model.Run`` lives in the external clone, not in the reference tree, so parity with the clone's own merge is unpinned.
There is no CPU fallback for the device entries.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from .utils_manet import ProbStore, torch_ptr

MAX_OBJECTS = 126             # ivosw_ipn_dilate: labels are int8 and -1 is taken
MAX_CHANNELS = 32             # ivosw_ipn_merge


# ----------------------------------------------------------------------------------------------- small host functions
def ToCudaVariable(xs, requires_grad=False):
    """utils/utils_ipn.py:11-15: every tensor of ``xs`` as a leaf on the GPU when there is one, where it is otherwise."""
    on_gpu = torch.cuda.is_available()
    return [(x.cuda() if on_gpu else x).detach().requires_grad_(requires_grad) for x in xs]


def ToCudaPN(mask):
    """utils/utils_ipn.py:18-23: the positive (== 1) and negative (== 0) scribble planes of a numpy mask, float32 [1, ...]."""
    planes = [torch.from_numpy((mask == v).astype(np.float32)).unsqueeze(0).float() for v in (1, 0)]
    return ToCudaVariable(planes)


def Get_weight(target, prev_targets, num_frames, at_least=-1):
    """utils/utils_ipn.py:37-72, in Python floats exactly as there: ``(left_end, right_end, weight)``; ``weight[f]`` is the share of
    the new estimate in frame f - 1 at ``target`` and wherever no earlier annotated frame lies on that side, else falling linearly to 0
    at the nearest one (at least ``at_least`` frames away, clipped to the video)."""
    later = [f for f in prev_targets if f > target]
    earlier = [f for f in prev_targets if f < target]
    right_end = min(later) if later else num_frames - 1
    left_end = max(earlier) if earlier else 0
    if (right_end - target) < at_least:
        right_end = min(target + at_least, num_frames - 1)
    if (target - left_end) < at_least:
        left_end = max(target - at_least, 0)
    weight = num_frames * [1.0]
    if later:
        step = 1.0 / (right_end - target)
        for n, f in enumerate(range(target + 1, num_frames)):
            weight[f] = max(0.0, 1.0 - (n + 1) * step)
    if earlier:
        step = 1.0 / (target - left_end)
        for n, f in enumerate(reversed(range(0, target))):
            weight[f] = max(0.0, 1.0 - (n + 1) * step)
    return left_end, right_end, weight


def weights32(weight):
    """``(w_new32, w_old32)`` float32 arrays: ``float32(w)`` and ``float32(1 - float64(w))`` - what torch makes of the Python scalars
    ``w`` and ``1 - w`` against a float32 tensor (the rule of ``alpha_beta32`` in tests/atnet_ref.py)."""
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(w.astype(np.float32)), np.ascontiguousarray((1 - w).astype(np.float32))


# ----------------------------------------------------------------------------------------------- dilation
def dilate_scribbles(mask_i8_dev, num_objects):
    """int8 [n,H,W] (or [H,W]) scribble maps on the device -> their dilation, same shape, one launch for the batch."""
    m = mask_i8_dev
    if not isinstance(m, torch.Tensor) or m.dtype != torch.int8:
        raise TypeError("dilate_scribbles: the scribble maps must be a torch.int8 tensor")
    if m.dim() not in (2, 3) or min(m.shape) < 1:
        raise ValueError(f"dilate_scribbles: the scribble maps must be [n,H,W] or [H,W], got {tuple(m.shape)}")
    if not 0 <= int(num_objects) <= MAX_OBJECTS:
        raise ValueError(f"dilate_scribbles: num_objects {num_objects} outside [0, {MAX_OBJECTS}]")
    if not m.is_cuda:
        raise RuntimeError("dilate_scribbles: the scribble maps must be a CUDA tensor (no CPU fallback)")
    m = m.contiguous()
    out = torch.empty_like(m)
    n = int(m.shape[0]) if m.dim() == 3 else 1
    L.check(L.lib().ivosw_ipn_dilate(L.dptr(m), n, int(m.shape[-2]), int(m.shape[-1]), int(num_objects), L.dptr(out),
                                     L.stream_ptr(m.device)), "ipn_dilate")
    return out


def Dilate_mask(mask, num_objects, device=None):
    """Drop-in for utils/utils_ipn.py:26-34: a sparse indexed numpy mask [H,W] (ignore = -1) in, its dilation as int64 numpy out,
    through ``ivosw_ipn_dilate``.  ``device``: the GPU to run on (default: the current one).  The kernel's diamond maximum equals the
    reference's loop as checked against scipy's ``binary_dilation`` per object; parity with cv2 itself is restated, not recorded."""
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.size < 1 or mask.dtype.kind not in "iu":
        raise ValueError(f"Dilate_mask: an integer [H,W] mask is expected, got {mask.dtype} {mask.shape}")
    if not 0 <= int(num_objects) <= MAX_OBJECTS:
        raise ValueError(f"Dilate_mask: num_objects {num_objects} outside [0, {MAX_OBJECTS}]")
    if not torch.cuda.is_available():
        raise RuntimeError("Dilate_mask: runs on the MI355X only (no CPU fallback)")
    m8 = np.where((mask >= 0) & (mask <= int(num_objects)), mask, -1).astype(np.int8)      # no (mask == o) of the reference sees the rest
    dev = torch.device("cuda" if device is None else device)
    return dilate_scribbles(torch.from_numpy(m8).to(dev), num_objects).cpu().numpy().astype(np.int64)


# ----------------------------------------------------------------------------------------------- merge, labels, all_P
class IpnStore(ProbStore):
    """A ProbStore for an IPN session of ``n_channels`` = objects + background channels: ``labels_u8`` [n, H, W], ``final_masks``
    [n, H, W] fp32 and ``buf`` [K, n, H, W], the estimate in canonical channel order, of which ``all_P`` is the permuted view.
    ``all_E`` wraps an estimate the adapter owns ([K, n, H, W] or IPN's [1, K, n, H, W], fp32 contiguous); without one the store
    allocates it (zeros).  ``merge_round`` binds ``buf`` to the merged estimate ITSELF when the channel order is the identity - no copy -
    and to a buffer of the store's own, made at the first such call, when it is not.
    ``probs=False`` makes a label-only store for ``masks=labels`` sessions: no ``buf``, the kernel gets a NULL probability pointer,
    and ``all_P`` is the LabelMasks of the label map."""

    def __init__(self, n_frames, n_channels, h, w, device, probs=True, all_E=None):
        if min(int(n_frames), int(n_channels), int(h), int(w)) < 1:
            raise ValueError("IpnStore: n_frames, n_channels, h and w must be positive")
        if int(n_channels) > MAX_CHANNELS:
            raise ValueError(f"IpnStore: at most {MAX_CHANNELS} channels")
        self.shape = (int(n_channels), int(n_frames), int(h), int(w))
        self.probs = bool(probs)
        self.all_E = None
        if all_E is not None:
            self.all_E = estimate_view(all_E, self.shape, "IpnStore")
        elif probs:
            self.all_E = torch.zeros(self.shape, dtype=torch.float32, device=device)
        self.buf = self.all_E if probs else None
        self.own = None                                   # the canonical copy, when a channel order needs one
        self.labels_u8 = torch.zeros(self.shape[1:], dtype=torch.uint8, device=device)
        self.final_masks = torch.zeros(self.shape[1:], dtype=torch.float32, device=device)

    @property
    def all_P(self):
        if self.buf is None:
            from ..models.assessment import LabelMasks
            return LabelMasks(self.labels_u8)
        return self.buf.permute(1, 0, 2, 3)


def estimate_view(E, shape, who):
    """IPN's estimate as [K,T,H,W]: a float32 contiguous tensor of that shape or with the batch axis 1 in front (a view, never a copy:
    the merge is in place)."""
    if not isinstance(E, torch.Tensor) or E.dtype != torch.float32:
        raise TypeError(f"{who}: the estimate must be a torch.float32 tensor")
    if E.dim() == 5 and E.shape[0] == 1:
        E = E[0]
    if E.dim() != 4 or min(E.shape) < 1 or (shape is not None and tuple(E.shape) != tuple(shape)):
        want = "[K,T,H,W] or [1,K,T,H,W]" if shape is None else f"{list(shape)} (or with a batch axis of 1)"
        raise ValueError(f"{who}: the estimate must be {want}, got {tuple(E.shape)}")
    if not E.is_contiguous():
        raise ValueError(f"{who}: the estimate must be contiguous (it is read, and merged, in place)")
    return E.detach()


def check_index(index, K, who):
    """``index`` (None = identity) as a list; raises unless it is a permutation of 0 .. K-1.  index[j] = the canonical channel at j."""
    if index is None:
        return list(range(K))
    index = [int(v) for v in index]
    if sorted(index) != list(range(K)):
        raise ValueError(f"{who}: index {index} is not a permutation of 0 .. {K - 1}")
    return index


def merge_call(E, prev, w32, index, probs, probs_stride_c, label_u8, label_f32):
    """ivosw_ipn_merge on [K,T,H,W] views; ``index`` a checked list; every output optional."""
    K, T, H, W = (int(v) for v in E.shape)
    identity = index == list(range(K))
    fptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.check(L.lib().ivosw_ipn_merge(
        L.dptr(E), L.dptr(prev) if prev is not None else None, K, T, H, W, fptr(w32[0]) if prev is not None else None,
        fptr(w32[1]) if prev is not None else None, None if identity else L.int_array(index),
        L.dptr(probs) if probs is not None else None, int(probs_stride_c), L.dptr(label_u8) if label_u8 is not None else None,
        L.dptr(label_f32) if label_f32 is not None else None, L.stream_ptr(E.device)), "ipn_merge")


def merge_round(all_E, prev_E, weight, index, store):
    """One interaction's end, ONE kernel call: ``all_E`` (this interaction's estimate, [1,K,T,H,W] or [K,T,H,W] fp32 on the device)
    becomes ``w * all_E + (1 - w) * prev_E`` per frame IN PLACE (``weight``: the T values of ``Get_weight``; ``prev_E = None``: the first
    interaction, nothing is blended and ``weight`` is not read), the store's ``labels_u8`` and ``final_masks`` take the labels
    (``To_np_label``'s rule) and its ``buf`` the canonical estimate.  Returns ``(final_masks, all_P)`` as ``get_results`` does: ``all_P``
    [T,K,H,W] is a permuted view of ``all_E`` itself when ``index`` is the identity (None), of the store's own buffer otherwise, and the
    LabelMasks of the label map for a label-only store."""
    if not isinstance(store, IpnStore):
        raise TypeError("merge_round: store must be an IpnStore")
    E = estimate_view(all_E, store.shape, "merge_round")
    K, T, H, W = store.shape
    prev = w32 = None
    if prev_E is not None:
        prev = estimate_view(prev_E, store.shape, "merge_round (prev_E)")
        w32 = weights32(weight)
        if w32[0].size != T:
            raise ValueError(f"merge_round: {w32[0].size} weights for {T} frames")
    index = check_index(index, K, "merge_round")
    if store.labels_u8.device != E.device or (prev is not None and prev.device != E.device):
        raise ValueError("merge_round: the estimates and the store are on different devices")
    if not E.is_cuda:
        raise RuntimeError("merge_round: the estimates must be CUDA tensors (no CPU fallback)")
    probs = None
    if store.probs and index != list(range(K)):
        if store.own is None:
            store.own = torch.empty(store.shape, dtype=torch.float32, device=E.device)
        probs = store.own
    merge_call(E, prev, w32, index, probs, T * H * W, store.labels_u8, store.final_masks)
    store.all_E = E
    if store.probs:
        store.buf = E if probs is None else probs
    return store.final_masks, store.all_P


def To_np_label(all_E, K, index):
    """Drop-in for utils/utils_ipn.py:75-81: IPN's estimate [1,K,T,H,W] (fp32, on the device) in, the uint8 numpy label map [T,H,W] out
    (the first maximum over the canonical channels), through ``ivosw_ipn_merge`` and ONE uint8 copy - the float estimate stays where
    it is.  ``index``: the list the reference takes (index[j] = the canonical channel at position j)."""
    E = estimate_view(all_E, None, "To_np_label")
    if int(K) != E.shape[0]:
        raise ValueError(f"To_np_label: K = {K} but the estimate has {E.shape[0]} channels")
    index = check_index(index, int(K), "To_np_label")
    if not E.is_cuda:
        raise RuntimeError("To_np_label: the estimate must be a CUDA tensor (no CPU fallback)")
    label = torch.empty(E.shape[1:], dtype=torch.uint8, device=E.device)
    merge_call(E, None, None, index, None, 0, label, None)
    return label.cpu().numpy()
