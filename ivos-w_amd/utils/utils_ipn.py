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
* the overlays (``overlay_davis`` :113-128, ``checkerboard`` / ``BIG_BOARD`` :131-143, ``overlay_checker`` :146-157, ``overlay_color``
  :160-171, ``overlay_fade`` :174-190): the reference blends one whole image per object in float64 on the CPU and finds the contour
  with ``scipy.ndimage.binary_dilation``; ``overlay_session`` renders any list of a session's frames from the frames and the label map
  that already sit on the device with ONE ``ivosw_overlay_frames`` call (``csrc/overlay.hip``), bit for bit what the reference
  functions give on uint8 images (tests/golden/overlay_fixtures.npz).  The four functions of the reference's names are drop-ins
  around the same kernel with one frame.  The reference's board stops at 1000 pixels a side (a larger image raises there); here the
  checker pattern simply continues.  Float images are not restated: a non-uint8 image is a TypeError.

* the scribble input (eval_agent_ipn.py: ``scribbles2mask`` at full resolution, then ``Dilate_mask``): ``scribble_input`` draws the
  annotated frame's paths on the device (``csrc/scribble.hip``, ``utils/scribbles.py``) and dilates the map where it lies.

There is no CPU fallback for the device entries.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from .utils_manet import ProbStore, torch_ptr

MAX_OBJECTS = 126             # ivosw_ipn_dilate: labels are int8 and -1 is taken
MAX_CHANNELS = 32             # ivosw_ipn_merge
MAX_OVERLAY_OBJECTS = 32      # ivosw_overlay_frames
OVERLAY_STYLES = {"davis": L.OVERLAY_DAVIS, "fade": L.OVERLAY_FADE, "checker": L.OVERLAY_CHECKER, "color": L.OVERLAY_COLOR}


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


def scribble_input(scribbles, frame, size, num_objects, device=None):
    """``Dilate_mask(scribbles2mask(scribbles, size)[frame], num_objects)`` on the device: the int8 map [H,W] of ``frame`` drawn by
    ``ivosw_scribble_raster`` (that frame's paths only) and dilated by ``ivosw_ipn_dilate`` - three launches, no host array, no
    synchronisation.  The line rule is this project's (utils/scribbles.py)."""
    from . import scribbles as S
    if not 0 <= int(num_objects) <= MAX_OBJECTS:
        raise ValueError(f"scribble_input: num_objects {num_objects} outside [0, {MAX_OBJECTS}]")
    m = S.scribble_maps(scribbles, size, frames=[int(frame)], device=device)
    return dilate_scribbles(m, num_objects)[0]


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


# ----------------------------------------------------------------------------------------------- overlays
def davis_palette(n=MAX_OVERLAY_OBJECTS):
    """The DAVIS / PASCAL-VOC colour map for objects 1 .. n, uint8 [n,3]: bit j of the object id goes to bit 7 - j // 3 of channel
    j % 3 (object 1 = (128, 0, 0), 2 = (0, 128, 0), 3 = (128, 128, 0), ...)."""
    pal = np.zeros((int(n), 3), dtype=np.uint8)
    for o in range(1, int(n) + 1):
        for j in range(24):
            pal[o - 1, j % 3] |= ((o >> j) & 1) << (7 - j // 3)
    return pal


def overlay_options(style, n_objects, select=0, alpha=0.5, palette=None, color=(255, 0, 255)):
    """The checked ``ivosw_overlay_t`` of a call (``_lib.Overlay``); ``palette`` None = ``davis_palette()``, else up to 32 rows of uint8
    RGB (object i + 1 takes row i; missing rows are black)."""
    if not isinstance(style, str) or style not in OVERLAY_STYLES:
        raise ValueError(f"overlay: style must be one of {sorted(OVERLAY_STYLES)}, got {style!r}")
    n_objects, select, alpha = int(n_objects), int(select), float(alpha)
    if not 1 <= n_objects <= MAX_OVERLAY_OBJECTS:
        raise ValueError(f"overlay: n_objects {n_objects} outside [1, {MAX_OVERLAY_OBJECTS}]")
    if not 0 <= select <= n_objects:
        raise ValueError(f"overlay: select {select} outside [0, {n_objects}]")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"overlay: alpha {alpha} not in [0, 1]")
    pal = np.zeros((MAX_OVERLAY_OBJECTS, 3), dtype=np.uint8)
    rows = davis_palette() if palette is None else np.array(palette, dtype=np.uint8)
    if rows.ndim != 2 or rows.shape[1] != 3 or rows.shape[0] > MAX_OVERLAY_OBJECTS:
        raise ValueError(f"overlay: palette must be uint8 [k,3] with k <= {MAX_OVERLAY_OBJECTS}, got {rows.shape}")
    pal[:rows.shape[0]] = rows
    col = np.array(color, dtype=np.uint8).reshape(-1)
    if col.size != 3:
        raise ValueError("overlay: color must be three uint8 values")
    opt = L.Overlay(style=OVERLAY_STYLES[style], n_objects=n_objects, select=select, alpha=alpha)
    ctypes.memmove(opt.palette, pal.ctypes.data, pal.nbytes)
    ctypes.memmove(opt.color, col.ctypes.data, 3)
    return opt


def overlay_session(frames, labels, n_objects, style="davis", frame_ids=None, select=0, alpha=0.5, palette=None, color=(255, 0, 255),
                    out="rgb"):
    """The pictures of a session on the device, ONE ``ivosw_overlay_frames`` call, no synchronisation: ``frames`` (a float32 [n,3,H,W]
    video on the device or a ``PackedFrames``) with ``labels`` (a device uint8 [n,H,W] label map or a ``LabelMasks``; value i + 1 is
    object i) drawn on them in ``style`` ("davis", "fade", "checker", "color").  ``frame_ids``: the frames to render, any order, repeats
    allowed (None: all, in order).  ``select``: 0 draws every object 1 .. n_objects, o draws object o alone.  Returns a device uint8
    tensor [m,H,W,3] (``out="rgb"``: what numpy and an image encoder take) or [m,H,W,4] (``out="rgbx"``, byte 3 = 0)."""
    from ..models.assessment import LabelMasks, PackedFrames
    if out not in ("rgb", "rgbx"):
        raise ValueError(f"overlay_session: out must be 'rgb' or 'rgbx', got {out!r}")
    opt = overlay_options(style, n_objects, select, alpha, palette, color)
    if isinstance(frames, PackedFrames):
        fr, kind, (n, H, W) = frames.rgbx, L.FRAMES_RGBX8, (frames.n, frames.H, frames.W)
    else:
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
            raise TypeError("overlay_session: frames must be a float32 [n,3,H,W] tensor or a PackedFrames")
        fr, kind, (n, H, W) = frames.contiguous(), L.FRAMES_F32, (int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[3]))
    lab = labels.map if isinstance(labels, LabelMasks) else labels
    if not isinstance(lab, torch.Tensor) or lab.dtype != torch.uint8 or tuple(lab.shape) != (n, H, W):
        raise TypeError(f"overlay_session: labels must be a uint8 [{n},{H},{W}] tensor or a LabelMasks of that shape")
    if not fr.is_cuda or not lab.is_cuda:
        raise RuntimeError("overlay_session: frames and labels must be CUDA tensors (no CPU fallback)")
    if fr.device != lab.device:
        raise ValueError("overlay_session: frames and labels are on different devices")
    lab = lab.contiguous()
    ids = None
    if frame_ids is not None:
        ids = [int(f) for f in frame_ids]
        if not ids or min(ids) < 0 or max(ids) >= n:
            raise ValueError(f"overlay_session: frame_ids must be a non-empty list of frames in [0, {n}), got {ids}")
    m = n if ids is None else len(ids)
    pics = torch.empty((m, H, W, 4 if out == "rgbx" else 3), dtype=torch.uint8, device=fr.device)
    L.check(L.lib().ivosw_overlay_frames(L.dptr(fr), kind, L.dptr(lab), n, H, W, None if ids is None else L.int_array(ids), m,
                                         ctypes.byref(opt), L.dptr(pics), L.OUT_RGBX8 if out == "rgbx" else L.OUT_RGB8,
                                         L.stream_ptr(fr.device)), "overlay_frames")
    return pics


def _overlay_image(who, image, mask, style, device=None, **kw):
    """One numpy uint8 [H,W,3] image and the binary mask ``mask == 1`` through the kernel, one frame; numpy of the image's dtype back."""
    from ..models.assessment import PackedFrames
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise TypeError(f"{who}: a uint8 image is expected, got {image.dtype} (the reference's float-image behaviour is not restated)")
    if image.ndim != 3 or image.shape[2] != 3 or image.size < 1:
        raise ValueError(f"{who}: an [H,W,3] image is expected, got {image.shape}")
    binary = np.asarray(mask) == 1
    if binary.shape != image.shape[:2]:
        raise ValueError(f"{who}: the mask {binary.shape} does not fit the image {image.shape[:2]}")
    overlay_options(style, 1, 1, **kw)                                       # (bad options are refused before the GPU is touched)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: runs on the MI355X only (no CPU fallback)")
    dev = torch.device("cuda" if device is None else device)
    rgbx = np.zeros(image.shape[:2] + (4,), dtype=np.uint8)
    rgbx[..., :3] = image
    pics = overlay_session(PackedFrames(torch.from_numpy(rgbx[None]).to(dev)), torch.from_numpy(binary.astype(np.uint8)[None]).to(dev), 1,
                           style=style, select=1, **kw)
    return pics[0].cpu().numpy().astype(image.dtype)


def overlay_davis(image, mask, rgb=[255, 0, 0], cscale=2, alpha=0.5, device=None):
    """Drop-in for utils/utils_ipn.py:113-128 on uint8 images: inside ``mask == 1`` each channel is trunc(v * alpha + (1 - alpha) * c),
    the mask's contour is black.  ``cscale`` is accepted and ignored, as in the reference."""
    return _overlay_image("overlay_davis", image, mask, "davis", device, alpha=alpha, palette=[rgb])


def overlay_fade(image, mask, device=None):
    """Drop-in for utils/utils_ipn.py:174-190 on uint8 images: outside ``mask == 1`` each channel is trunc(0.4 * v), the contour is
    (0, 255, 255)."""
    return _overlay_image("overlay_fade", image, mask, "fade", device)


def overlay_checker(image, mask, device=None):
    """Drop-in for utils/utils_ipn.py:146-157 on uint8 images: outside ``mask == 1`` the 20-pixel checkerboard of 223 and 32 (BIG_BOARD;
    the reference raises above 1000 pixels a side, here the pattern continues)."""
    return _overlay_image("overlay_checker", image, mask, "checker", device)


def overlay_color(image, mask, rgb=[255, 0, 255], device=None):
    """Drop-in for utils/utils_ipn.py:160-171 on uint8 images: outside ``mask == 1`` the colour ``rgb``."""
    return _overlay_image("overlay_color", image, mask, "color", device, color=rgb)
