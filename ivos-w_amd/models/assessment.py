"""Segmentation-quality-assessment network on the MI355X — drop-in for the reference's ``models.assessment``.

Same class surface and ``state_dict`` (326 tensors) as /root/reference/models/assessment.py (``Encoder`` :12-63,
``AssessNet`` :66-182); ``forward(tf, tp)`` runs entirely in libivosw_hip.so:

  mask bbox (wavefront min/max, no D2H)  ->  fused ROI bilinear resample + (f-mean)/std to NHWC4
  ->  stem 7x7 (RGB|mask concatenated) + BN + ReLU  ->  max-pool  ->  16 bottlenecks as implicit-GEMM MFMA
  convolutions with folded BN / residual / ReLU epilogues  ->  8x8 average pool + fc1.

The torch modules below are parameter containers only (keys, shapes, checkpoint I/O); torchvision is not
needed and nothing is downloaded.  ``precision='fp32'`` (default) is the parity mode (fp32 MFMA, scores within
1e-4 rtol of the reference CPU path); ``precision='bf16x3'`` keeps fp32 tensors and the 1e-4 bar but runs every contraction
- the stem included - as three bf16 MFMA passes on (hi, lo) splits (a b ~ ah bh + ah bl + al bh: error ~ 2^-17 per product, 16 / 3 of
the fp32 matrix rate); ``precision='bf16'`` is the throughput mode (bf16 operands, fp32 accumulate).
Inference only (eval-mode BatchNorm): training the trunk is outside this path (folded BatchNorm cannot represent it); the score head
fc1 is fitted on the device on the pooled features of the frozen trunk (``forward_features`` / ``fit_head`` / ``set_head``).
"""
import ctypes
import os
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L


class _Bottleneck(nn.Module):
    """Parameter container with torchvision's ResNet bottleneck attribute names."""

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))
        else:
            self.downsample = None


def _stage(inplanes, planes, blocks, stride):
    layers = [_Bottleneck(inplanes, planes, stride, True)]
    layers += [_Bottleneck(planes * 4, planes, 1, False) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


class Encoder(nn.Module):
    """ResNet-50 trunk + the extra 1-channel stems (conv1_m / conv1_n are unused upstream but part of the
    checkpoint, models/assessment.py:15-20)."""

    def __init__(self):
        super().__init__()
        self.conv1_m = nn.Conv2d(1, 64, 7, 2, 3, bias=True)
        self.conv1_p = nn.Conv2d(1, 64, 7, 2, 3, bias=False)
        self.conv1_n = nn.Conv2d(1, 64, 7, 2, 3, bias=False)
        for m in (self.conv1_m, self.conv1_p, self.conv1_n):
            fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            m.weight.data.normal_(0, math.sqrt(2.0 / fan))
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.res2 = _stage(64, 64, 3, 1)
        self.res3 = _stage(256, 128, 4, 2)
        self.res4 = _stage(512, 256, 6, 2)
        self.res5 = _stage(1024, 512, 3, 2)
        for m in [self.conv1] + [c for s in (self.res2, self.res3, self.res4, self.res5) for c in s.modules()
                                 if isinstance(c, nn.Conv2d)]:
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")   # no pretrained download
        self.register_buffer("mean", torch.FloatTensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.FloatTensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def forward(self, in_f, in_p, in_g=None):
        raise RuntimeError("Encoder has no standalone forward on the MI355X path; call AssessNet(tf, tp)")


_DTYPES = {"fp32": L.F32, "bf16": L.BF16, "bf16x3": L.F32X3}
_TAPS = {"roi": (1, (256, 256, 4)), "stem": (2, (128, 128, 64)), "pool": (3, (64, 64, 64)),
         "res2": (4, (64, 64, 256)), "res3": (5, (32, 32, 512)), "res4": (6, (16, 16, 1024)),
         "res5": (7, (8, 8, 2048)), "pooled": (8, (2048,))}


_LAYOUTS = {"hwc": (L.U8_HWC3, 3), "chw": (L.U8_CHW3, 1)}      # layout -> (IVOSW_U8_*, the axis that holds the 3 channels)


class PackedFrames:
    """The 8-bit frames of a video on the device in the library's RGBX8 format: ``rgbx`` uint8 [n,H,W,4], bytes R, G, B, 0.  The colour
    value of byte v is float32(v) / 255, so every AssessNet entry handed a PackedFrames computes bit for bit what it computes on
    ``to_float()`` - from a quarter of the bytes.  Build one with ``AssessNet.pack_frames`` / ``utils_agent.pack_video``."""

    def __init__(self, rgbx):
        if not isinstance(rgbx, torch.Tensor) or rgbx.dtype != torch.uint8:
            raise TypeError("PackedFrames holds a torch.uint8 tensor")
        if rgbx.dim() != 4 or rgbx.shape[3] != 4 or not rgbx.is_contiguous():
            raise ValueError(f"PackedFrames holds a contiguous [n,H,W,4] tensor, got {tuple(rgbx.shape)}")
        self.rgbx = rgbx
        self.n, self.H, self.W = (int(v) for v in rgbx.shape[:3])

    @property
    def device(self):
        return self.rgbx.device

    def __len__(self):
        return self.n

    def to_float(self):
        """float32 [n,3,H,W] in 0..1: what the float entry points take.  The 256 values float32(v) / 255 come from a table divided on the
        host: on the device torch divides a tensor by a scalar as a product with float32(1 / 255), which rounds 95 / 255 (and more)
        one ulp away from the division that defines the format."""
        table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.)).to(self.rgbx.device)
        idx = self.rgbx[..., :3].permute(0, 3, 1, 2).contiguous().view(-1).to(torch.int32)
        return table.index_select(0, idx).view(self.n, 3, self.H, self.W)


def pack_frames(u8, device, layout="hwc"):
    """Decoded 8-bit frames -> PackedFrames on ``device``.  u8: torch.uint8 tensor or numpy uint8 array, [n,H,W,3] (layout "hwc": cv2 /
    PIL after the channel flip) or [n,3,H,W] ("chw"), on the host or the device.  A host input is uploaded as bytes; the packing is one
    launch of ivosw_frames_pack_u8 on the device."""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if isinstance(u8, np.ndarray):
        if u8.dtype != np.uint8:
            raise TypeError(f"8-bit frames must be uint8, got {u8.dtype}")
        u8 = torch.from_numpy(np.ascontiguousarray(u8))
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8:
        raise TypeError(f"8-bit frames must be a torch.uint8 tensor or a numpy uint8 array, got {getattr(u8, 'dtype', type(u8))}")
    code, axis = _LAYOUTS[layout]
    if u8.dim() != 4 or u8.shape[axis] != 3 or min(u8.shape) < 1:
        want = "[n,H,W,3]" if layout == "hwc" else "[n,3,H,W]"
        raise ValueError(f"layout {layout!r} takes {want}, got {tuple(u8.shape)}")
    n, H, W = (int(u8.shape[i]) for i in range(4) if i != axis)
    src = u8.detach().to(device).contiguous()
    rgbx = torch.empty(n, H, W, 4, dtype=torch.uint8, device=src.device)
    L.check(L.lib().ivosw_frames_pack_u8(L.dptr(src), code, n, H, W, L.dptr(rgbx), L.stream_ptr(src.device)), "frames_pack_u8")
    return PackedFrames(rgbx)


MASK_KINDS = ("float32", "labels")


class LabelMasks:
    """The masks of a video as ONE hard label map on the device: ``map`` uint8 [n,H,W], value i + 1 = object i, 0 (and any value above
    the number of objects) = no object - the format ivosw_seg_epilogue writes and ivosw_jf_counts reads.  Hand one to AssessNet /
    utils_agent wherever an ``all_P`` is accepted: the plane of (frame, object i) is then (map == i + 1) as 1.0 / 0.0, and every result
    is bit for bit what the float path gives on ``to_planes()`` - from 1 byte per pixel and frame instead of 4 * (objects + 1).
    Only this type selects the label path: a plain uint8 tensor in all_P's place is cast to float as before.
    The two last dimensions are made contiguous (a copy only if they are not); frames may be strided."""

    def __init__(self, map):
        if not isinstance(map, torch.Tensor) or map.dtype != torch.uint8:
            raise TypeError("LabelMasks holds a torch.uint8 tensor")
        if map.dim() != 3 or min(map.shape) < 1:
            raise ValueError(f"LabelMasks holds a [n,H,W] tensor, got {tuple(map.shape)}")
        n, H, W = (int(v) for v in map.shape)
        if map.stride(2) != 1 or map.stride(1) != W or (n > 1 and map.stride(0) < H * W):
            map = map.contiguous()
        self.map = map
        self.n, self.H, self.W = n, H, W

    @property
    def device(self):
        return self.map.device

    @property
    def is_cuda(self):
        return self.map.is_cuda

    def __len__(self):
        return self.n

    def to(self, device):
        """The same masks on ``device`` (self when they are there already)."""
        device = torch.device(device)
        return self if self.map.device == device else LabelMasks(self.map.to(device))

    @classmethod
    def from_probs(cls, all_P):
        """all_P [n,C,H,W] (channel 0 = background, channel i + 1 = object i) -> its hard labels, ``all_P.argmax(1)`` with the FIRST
        maximum on ties.  This DISCARDS the soft values: the float path scores the probabilities themselves (it thresholds them at
        0.5 for the box and samples them for the tile), the label path scores the one-hot planes of the argmax."""
        if not isinstance(all_P, torch.Tensor) or all_P.dim() != 4:
            raise ValueError("from_probs takes all_P [n,C,H,W]")
        if all_P.shape[1] > 256:
            raise ValueError(f"a label map holds at most 255 objects, all_P has {all_P.shape[1] - 1}")
        if all_P.is_cuda:
            lab = all_P.argmax(1)
        else:                                    # numpy's argmax names the first maximum by definition
            lab = torch.from_numpy(np.argmax(all_P.detach().numpy(), axis=1))
        return cls(lab.to(torch.uint8))

    def to_planes(self, n_obj):
        """The one-hot float32 [n, n_obj + 1, H, W] the label path is defined on: channel i + 1 = (map == i + 1), channel 0 = everything
        else (label 0 and labels above n_obj).  For tests and fallbacks: 4 * (n_obj + 1) times the map's bytes."""
        n_obj = int(n_obj)
        if not 1 <= n_obj <= 255:
            raise ValueError(f"n_obj must be 1 .. 255, got {n_obj}")
        m = self.map[:, None].to(torch.int64)
        obj = (m == torch.arange(1, n_obj + 1, device=self.map.device).view(1, n_obj, 1, 1)).to(torch.float32)
        return torch.cat([1.0 - obj.sum(1, keepdim=True), obj], 1)


class ScoreCache:
    """What one video's session keeps between interactions for the incremental forward (``AssessNet.forward_videos_incremental``): the
    planes it was last scored on (``planes``: dense [n_obj, n_frames, H*W] fp32 on the device, unit order), the score table
    (``scores`` [n_obj, n_frames]) and a key - the identity of the frames object (held by a STRONG reference, as utils_agent._FrameCache
    holds its host tensor, so the allocator cannot hand its address to another video while the entry lives), n_frames, n_obj, H, W, and
    the net's precision and ``_weights_key()``.  For a LabelMasks session ``planes`` is a uint8 [n_frames, H*W] copy of the map
    instead, and the mask kind is part of the key.  Any mismatch makes the cache cold: every unit is scored again.  The key guards what the
    device comparison cannot see (other frames, other weights); the masks are compared bit for bit against whatever planes the cache
    holds, so a wrong guess about "same session" costs time, never results.  Frames rewritten in place behind an unchanged tensor
    object (through numpy, or .data) are not seen: drop the cache then (``utils_agent.clear_score_cache``).
    ``units`` / ``rescored``: the video's units and how many of them the last call scored again."""

    def __init__(self):
        self.planes, self.scores, self.key, self.src = None, None, None, None
        self.units, self._rescored = 0, 0

    @staticmethod
    def make_key(net, frames, n_frames, n_obj, H, W, masks="float32"):
        """(key, src): src is the object whose identity stands for the frames.  masks: the kind of the session's masks (MASK_KINDS)."""
        if masks not in MASK_KINDS:
            raise ValueError(f"masks must be 'float32' or 'labels', got {masks!r}")
        src = frames
        t = frames.rgbx if isinstance(frames, PackedFrames) else frames
        ident = (t.data_ptr(), t._version) if isinstance(t, torch.Tensor) else ()
        return (id(src), ident, int(n_frames), int(n_obj), int(H), int(W), net.precision, net._weights_key(), masks), src

    @staticmethod
    def nbytes_for(n_frames, n_obj, H, W, masks="float32"):
        """Device bytes of a bound cache: the copy of the masks (fp32 planes per unit, or one uint8 map per frame) plus the score table."""
        if masks not in MASK_KINDS:
            raise ValueError(f"masks must be 'float32' or 'labels', got {masks!r}")
        n_frames, n_obj, plane = int(n_frames), int(n_obj), int(H) * int(W)
        if masks == "labels":
            return n_frames * plane + 4 * n_frames * n_obj
        return 4 * n_frames * n_obj * (plane + 1)

    @property
    def nbytes(self):
        return 0 if self.key is None else self.nbytes_for(*self.key[2:6], masks=self.key[8])

    @property
    def rescored(self):
        if isinstance(self._rescored, torch.Tensor):                # a multi-video call: counted on the device, fetched when asked for
            self._rescored = int(self._rescored.item())
        return self._rescored

    def bind(self, net, frames, n_frames, n_obj, H, W, device, masks="float32"):
        """Make the cache one for this video; returns True when it is cold (its planes and scores are undefined).  Switching the mask
        kind changes the key: the cache turns cold and its copy is reallocated in the other format."""
        key, src = self.make_key(net, frames, n_frames, n_obj, H, W, masks)
        device = torch.device(device)
        warm = (self.key == key and self.src is src and self.planes is not None and self.planes.device == device)
        if not warm:
            numel, dt = (n_frames * H * W, torch.uint8) if masks == "labels" else (n_obj * n_frames * H * W, torch.float32)
            if self.planes is None or self.planes.device != device or self.planes.numel() != numel or self.planes.dtype != dt:
                self.planes = torch.empty(numel, dtype=dt, device=device)
            self.scores = torch.empty(n_obj, n_frames, dtype=torch.float32, device=device)
            self.key, self.src = key, src
        self.units = n_obj * n_frames
        return not warm

    def clear(self):
        self.planes, self.scores, self.key, self.src = None, None, None, None
        self.units, self._rescored = 0, 0


class HeadFitResult:
    """What ``AssessNet.fit_head`` returns.  ``log``: the device tensor [n_configs, n_steps, 3] of every step's loss, diff and counter;
    ``epoch_loss`` / ``epoch_diff`` [n_configs, num_epochs] float64: their means over the steps of an epoch that were taken (the
    reference's ``* Epoch`` line); ``w`` [n_configs,2048], ``b`` [n_configs]: the fitted heads (host, fp32); with a holdout
    ``holdout_loss`` / ``holdout_diff`` / ``holdout_n`` [n_configs]: one eval-only pass over the held-out rows; ``best``: the config
    with the lowest held-out loss (without held-out rows: the lowest last-epoch loss); ``configs``: the hyper-parameters as run."""

    def chosen(self):
        return self.w[self.best], self.b[self.best]


class AssessNet(nn.Module):
    def __init__(self, precision="fp32", chunk=0):
        super().__init__()
        if precision not in _DTYPES:
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        self.Encoder = Encoder()
        self.fc1 = nn.Linear(2048, 1)
        self.cnt = 0
        self.precision = precision
        self.chunk = chunk
        self._packed = None
        self._packed_key = None
        self._wver = 0                      # bumped whenever the weights can have changed (load_state_dict, .to(), ...)
        self._ws = L.Workspace()

    # ------------------------------------------------------------------ weights
    def invalidate_packed(self):
        """Call after modifying parameters in place by hand (load_state_dict / .to() / .float() do it themselves)."""
        self._wver += 1

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._wver += 1
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._wver += 1
        return out

    def _weights_key(self):
        # O(1): a forward at eval sizes (B ~ 100 frames) is ~1.6 ms of GPU time, walking the 326 tensors of the
        # state_dict on every call cost a comparable amount of host time.  The first and last tensors stand guard
        # against in-place edits that bypass the counter.
        w0, w1 = self.Encoder.conv1.weight, self.fc1.weight
        key = (self.precision, self._wver, str(w1.device), w0.data_ptr(), w0._version, w1.data_ptr(), w1._version)
        if os.environ.get("IVOSW_WEIGHTS_KEY", "") == "full":
            # debug / safety switch: walk every tensor, so an in-place edit of ANY parameter or BN buffer that bypassed
            # load_state_dict / .to() / invalidate_packed() re-packs the weights (the O(1) key watches two tensors and a counter)
            key += tuple((t.data_ptr(), t._version) for t in self.state_dict().values())
        return key

    def _ensure_packed(self):
        key = self._weights_key()
        if self._packed is not None and key == self._packed_key:
            return self._packed
        dev = self.fc1.weight.device
        lib, dt = L.lib(), _DTYPES[self.precision]
        sd = self.state_dict()
        assert len(sd) == L.ASSESS_NTENSORS
        keep, ptrs = [], (ctypes.c_void_p * L.ASSESS_NTENSORS)()
        for i, (k, t) in enumerate(sd.items()):
            if not t.is_floating_point():              # num_batches_tracked
                ptrs[i] = None
                continue
            t32 = t.detach().to(torch.float32).contiguous()
            keep.append(t32)
            ptrs[i] = L.dptr(t32).value
        packed = torch.empty(int(lib.ivosw_assess_packed_bytes(dt)), dtype=torch.uint8, device=dev)
        L.check(lib.ivosw_assess_pack(L.dptr(packed), dt, ptrs, L.ASSESS_NTENSORS, L.stream_ptr(dev)), "assess_pack")
        torch.cuda.current_stream(dev).synchronize()   # `keep` temporaries may be freed after this
        self._packed, self._packed_key = packed, key
        return packed

    # ------------------------------------------------------------------ forward
    def _run(self, tf, tp, tap=None):
        if self.training:
            raise RuntimeError("AssessNet on the MI355X path is inference-only (eval-mode BatchNorm); call .eval() — "
                               "training AssessNet is outside the hot path")
        u8 = isinstance(tf, PackedFrames)                # the 8-bit path is reached through this type only: a plain uint8 tensor is cast
        if u8:
            B, H, W = tf.n, tf.H, tf.W
            tf = tf.rgbx
        else:
            tf = tf.detach().to(torch.float32).contiguous()
            B, C, H, W = tf.shape
            assert C == 3
        tp = tp.detach().to(torch.float32).contiguous()
        assert tuple(tp.shape) == (B, H, W)
        dev = tf.device
        packed = self._ensure_packed()
        lib, dt = L.lib(), _DTYPES[self.precision]
        chunk = B if tap else self.chunk
        nbytes = lib.ivosw_assess_ws_bytes(dt, B, H, W, chunk)
        ws = self._ws.get(nbytes, dev)
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        stage, tap_t = 0, None
        if tap:
            stage, shp = _TAPS[tap]
            tdt = torch.float32 if (tap == "pooled" or self.precision != "bf16") else torch.bfloat16
            tap_t = torch.empty((B,) + shp, dtype=tdt, device=dev)
        fwd = lib.ivosw_assess_forward_u8 if u8 else lib.ivosw_assess_forward
        L.check(fwd(L.dptr(packed), dt, L.dptr(tf), L.dptr(tp), B, H, W, L.dptr(scores), L.dptr(ws),
                    nbytes, chunk, stage, L.dptr(tap_t) if tap else None, L.stream_ptr(dev)),
                "assess_forward_u8" if u8 else "assess_forward")
        return scores, tap_t

    def forward(self, tf, tp):
        """tf [B,3,H,W] in [0,1] (or a PackedFrames: the 8-bit path), tp [B,H,W] soft mask -> quality [B,1] ((1,) when B == 1, like
        the reference's ``.squeeze()``, models/assessment.py:179)."""
        scores, _ = self._run(tf, tp)
        return scores if scores.shape[0] == 1 else scores[:, None]

    def pack_frames(self, u8, layout="hwc"):
        """8-bit frames ([n,H,W,3] or, with layout="chw", [n,3,H,W]; torch or numpy uint8, host or device) -> PackedFrames on this
        network's device."""
        return pack_frames(u8, self.fc1.weight.device, layout)

    def forward_objects(self, all_F, all_P, n_objects):
        """Scores of every (object, frame) unit of ONE video without replicating the frames: all_F [n,3,H,W] fp32 on the
        device, all_P [n,C,H,W] fp32 on the device (any layout whose [H,W] planes are contiguous, e.g. the object-major
        ProbStore view), channel i+1 = object i (utils/utils_agent.py:118-119).  all_F may be a PackedFrames (the 8-bit path).
        Returns [n_objects, n] fp32 on the device."""
        if self.training:
            raise RuntimeError("AssessNet on the MI355X path is inference-only; call .eval()")
        if isinstance(all_P, LabelMasks):                   # label-map masks: the table path with one video (the only one that reads them)
            return self.forward_videos([(all_F, all_P, n_objects)])[0]
        u8 = isinstance(all_F, PackedFrames)
        if u8:
            n, H, W = all_F.n, all_F.H, all_F.W
            all_F = all_F.rgbx
        else:
            n, C3, H, W = all_F.shape
            assert C3 == 3
            if all_F.dtype != torch.float32 or not all_F.is_contiguous():
                all_F = all_F.detach().to(torch.float32).contiguous()
        assert all_P.shape[0] == n and tuple(all_P.shape[2:]) == (H, W) and all_P.shape[1] > n_objects
        if all_P.dtype != torch.float32 or all_P.stride(3) != 1 or all_P.stride(2) != W:
            all_P = all_P.detach().to(torch.float32).contiguous()
        dev = all_F.device
        packed = self._ensure_packed()
        lib, dt = L.lib(), _DTYPES[self.precision]
        units = n * n_objects
        nbytes = lib.ivosw_assess_ws_bytes(dt, units, H, W, self.chunk)
        ws = self._ws.get(nbytes, dev)
        scores = torch.empty(n_objects, n, dtype=torch.float32, device=dev)
        masks = all_P[:, 1:]                                # a view: channel 0 is the background
        fwd = lib.ivosw_assess_forward_objects_u8 if u8 else lib.ivosw_assess_forward_objects
        L.check(fwd(L.dptr(packed), dt, L.dptr(all_F), n, ctypes.c_void_p(masks.data_ptr()),
                    all_P.stride(0), all_P.stride(1), n_objects, H, W, L.dptr(scores),
                    L.dptr(ws), nbytes, self.chunk, L.stream_ptr(dev)), "assess_forward_objects_u8" if u8 else "assess_forward_objects")
        return scores

    def _video_entry(self, k, video, keep):
        """One (all_F | PackedFrames, all_P | LabelMasks, n_objects) of forward_videos -> (L.Video, L.Labels, n), normalised by
        forward_objects' rules; tensors the descriptors point into are appended to `keep`.  The Labels entry of a float video is empty."""
        all_F, all_P, n_objects = video
        n_objects = int(n_objects)
        u8 = isinstance(all_F, PackedFrames)
        if u8:
            n, H, W = all_F.n, all_F.H, all_F.W
            all_F = all_F.rgbx
        else:
            n, C3, H, W = all_F.shape
            assert C3 == 3, f"video {k}: all_F must be [n,3,H,W]"
            if all_F.dtype != torch.float32 or not all_F.is_contiguous():
                all_F = all_F.detach().to(torch.float32).contiguous()
        kind = L.FRAMES_RGBX8 if u8 else L.FRAMES_F32
        if isinstance(all_P, LabelMasks):
            assert (all_P.n, all_P.H, all_P.W) == (n, H, W) and n_objects >= 1, f"video {k}: LabelMasks shape"
            if not all_P.is_cuda or all_P.device != all_F.device:
                raise RuntimeError(f"ivos_w_amd: video {k}: the label map must live on the frames' GPU (there is no CPU fallback)")
            keep += [all_F, all_P.map]
            return (L.Video(L.dptr(all_F).value, None, 0, 0, kind, n, n_objects, H, W),
                    L.Labels(all_P.map.data_ptr(), all_P.map.stride(0) if n > 1 else H * W), n)
        assert all_P.shape[0] == n and tuple(all_P.shape[2:]) == (H, W) and all_P.shape[1] > n_objects >= 1, f"video {k}: all_P shape"
        if all_P.dtype != torch.float32 or all_P.stride(3) != 1 or all_P.stride(2) != W:
            all_P = all_P.detach().to(torch.float32).contiguous()
        if not all_P.is_cuda or all_P.device != all_F.device:
            raise RuntimeError(f"ivos_w_amd: video {k}: all_P must live on the frames' GPU (there is no CPU fallback)")
        masks = all_P[:, 1:]                                # a view: channel 0 is the background
        keep += [all_F, all_P]
        return L.Video(L.dptr(all_F).value, masks.data_ptr(), all_P.stride(0), all_P.stride(1), kind, n, n_objects, H, W), L.Labels(None, 0), n

    def forward_videos(self, videos):
        """Scores of every (object, frame) unit of SEVERAL videos in one pass (ivosw_assess_forward_videos): ``videos`` is a sequence of
        (all_F | PackedFrames, all_P, n_objects), each as ``forward_objects`` takes them - every video its own length, frame size, frame
        format and all_P layout, all on this network's device.  Returns a list with one [n_objects, n] fp32 view per video, in the order
        given, all views of one flat score tensor in unit order (video-major, then object-major).  Each score is bit for bit what
        ``forward_objects`` gives for that video alone.  More than 32 videos run in groups of 32."""
        if self.training:
            raise RuntimeError("AssessNet on the MI355X path is inference-only; call .eval()")
        videos = list(videos)
        if not videos:
            return []
        keep, descs, labs, shapes = [], [], [], []
        for k, video in enumerate(videos):
            d, lab, n = self._video_entry(k, video, keep)
            descs.append(d)
            labs.append(lab)
            shapes.append((d.n_obj, n))
        dev = keep[0].device
        packed = self._ensure_packed()
        lib, dt = L.lib(), _DTYPES[self.precision]
        scores = torch.empty(sum(o * n for o, n in shapes), dtype=torch.float32, device=dev)
        off = 0
        for g in range(0, len(descs), L.MAX_VIDEOS):
            group, glab = descs[g:g + L.MAX_VIDEOS], labs[g:g + L.MAX_VIDEOS]
            arr = (L.Video * len(group))(*group)
            larr = (L.Labels * len(group))(*glab) if any(lab.map for lab in glab) else None       # the _lab entry only with a label video
            if larr is None:
                units = int(lib.ivosw_assess_videos_units(arr, len(group)))
                if units < 0:
                    L.check(units, "assess_videos_units")
            else:
                units = sum(d.n_frames * d.n_obj for d in group)
            nbytes = lib.ivosw_assess_ws_bytes(dt, units, group[0].H, group[0].W, self.chunk)     # (H, W are not looked at)
            ws = self._ws.get(nbytes, dev)
            out = scores[off:off + units]
            if larr is None:
                L.check(lib.ivosw_assess_forward_videos(L.dptr(packed), dt, arr, len(group), L.dptr(out), L.dptr(ws), nbytes, self.chunk,
                                                        0, None, L.stream_ptr(dev)), "assess_forward_videos")
            else:
                L.check(lib.ivosw_assess_forward_videos_lab(L.dptr(packed), dt, arr, larr, len(group), L.dptr(out), L.dptr(ws), nbytes,
                                                            self.chunk, 0, None, L.stream_ptr(dev)), "assess_forward_videos_lab")
            off += units
        views, off = [], 0
        for o, n in shapes:
            views.append(scores[off:off + o * n].view(o, n))
            off += o * n
        return views

    def forward_videos_incremental(self, videos, caches, sources=None):
        """``forward_videos`` that scores only the units whose mask planes changed since ``caches`` were last scored: ``caches`` holds one
        ``ScoreCache`` per video (distinct objects), ``sources`` optionally the object whose identity stands for each video's frames in
        the cache key (default: the all_F given; a caller that uploads a host video per call names the host tensor here).  Per group of
        up to 32 videos: ivosw_mask_delta_videos compares every plane with the cached one on the device and updates the cache, ONE
        4-byte device-to-host copy brings the number of dirty units - the one synchronisation this path adds to ``forward_videos`` -
        and ivosw_assess_forward_units scores those units into the full table.  Returns what ``forward_videos`` returns, bit for bit: one
        [n_objects, n] view per video of one flat score tensor in unit order.  ``cache.units`` / ``cache.rescored`` tell what the call
        did per video.  The masks may be rewritten in place between calls (ProbStore): the comparison is against the cache's own copy."""
        if self.training:
            raise RuntimeError("AssessNet on the MI355X path is inference-only; call .eval()")
        videos, caches = list(videos), list(caches)
        if len(videos) != len(caches) or len({id(c) for c in caches}) != len(caches):
            raise ValueError("forward_videos_incremental takes one distinct ScoreCache per video")
        sources = [v[0] for v in videos] if sources is None else list(sources)
        if not videos:
            return []
        keep, descs, labs, shapes = [], [], [], []
        for k, video in enumerate(videos):
            d, lab, n = self._video_entry(k, video, keep)
            descs.append(d)
            labs.append(lab)
            shapes.append((d.n_obj, n))
        dev = keep[0].device
        packed = self._ensure_packed()
        lib, dt, st = L.lib(), _DTYPES[self.precision], L.stream_ptr(dev)
        scores = torch.empty(sum(o * n for o, n in shapes), dtype=torch.float32, device=dev)
        off = 0
        for g in range(0, len(descs), L.MAX_VIDEOS):
            group, gc, glab = descs[g:g + L.MAX_VIDEOS], caches[g:g + L.MAX_VIDEOS], labs[g:g + L.MAX_VIDEOS]
            arr = (L.Video * len(group))(*group)
            larr = (L.Labels * len(group))(*glab) if any(lab.map for lab in glab) else None       # the _lab entries only with a label video
            if larr is None:
                units = int(lib.ivosw_assess_videos_units(arr, len(group)))
                if units < 0:
                    L.check(units, "assess_videos_units")
            else:
                units = sum(d.n_frames * d.n_obj for d in group)
            out = scores[off:off + units]
            cold, o = [], 0
            for d, lab, c, src in zip(group, glab, gc, sources[g:g + L.MAX_VIDEOS]):
                cold.append(c.bind(self, src, d.n_frames, d.n_obj, d.H, d.W, dev, masks="labels" if lab.map else "float32"))
                if not cold[-1]:
                    out[o:o + c.units].copy_(c.scores.view(-1))      # the table of the last call; the dirty entries are overwritten below
                o += c.units
            ptrs = (ctypes.c_void_p * len(group))(*[c.planes.data_ptr() for c in gc])
            meta = torch.empty(2 * units + 1, dtype=torch.int32, device=dev)       # [flags (units) | unit ids (units) | n_dirty]
            flags, ids, n_dirty = meta[:units], meta[units:2 * units], meta[2 * units:]
            if larr is None:
                L.check(lib.ivosw_mask_delta_videos(arr, len(group), ptrs, L.int_array(cold), L.dptr(flags), L.dptr(ids), L.dptr(n_dirty), st),
                        "mask_delta_videos")
            else:
                L.check(lib.ivosw_mask_delta_videos_lab(arr, larr, len(group), ptrs, L.int_array(cold), L.dptr(flags), L.dptr(ids),
                                                        L.dptr(n_dirty), st), "mask_delta_videos_lab")
            n_ids = int(n_dirty.item())                                 # the one synchronisation of the incremental path
            if n_ids:
                nbytes = lib.ivosw_assess_units_ws_bytes(dt, n_ids, self.chunk)
                ws = self._ws.get(nbytes, dev)
                if larr is None:
                    L.check(lib.ivosw_assess_forward_units(L.dptr(packed), dt, arr, len(group), L.dptr(ids), n_ids, L.dptr(out), L.dptr(ws),
                                                           nbytes, self.chunk, st), "assess_forward_units")
                else:
                    L.check(lib.ivosw_assess_forward_units_lab(L.dptr(packed), dt, arr, larr, len(group), L.dptr(ids), n_ids, L.dptr(out),
                                                               L.dptr(ws), nbytes, self.chunk, st), "assess_forward_units_lab")
            o = 0
            for c, was_cold in zip(gc, cold):
                c.scores.view(-1).copy_(out[o:o + c.units])
                c._rescored = n_ids if len(gc) == 1 else c.units if was_cold else flags[o:o + c.units].sum()
                o += c.units
            off += units
        views, off = [], 0
        for o, n in shapes:
            views.append(scores[off:off + o * n].view(o, n))
            off += o * n
        return views

    def forward_features(self, tf, tp):
        """``forward`` with the pooled features handed out (ivosw_assess_forward_features): -> (scores [B], features [B,2048] fp32), both
        on the device, no synchronisation.  Any B and chunk; the scores are ``forward``'s bit for bit, the features what fc1 is applied
        to - the rows ``fit_head`` fits on.  tf may be a PackedFrames (the 8-bit path)."""
        if self.training:
            raise RuntimeError("AssessNet on the MI355X path is inference-only (eval-mode BatchNorm); call .eval()")
        u8 = isinstance(tf, PackedFrames)
        if u8:
            B, H, W = tf.n, tf.H, tf.W
            tf = tf.rgbx
        else:
            tf = tf.detach().to(torch.float32).contiguous()
            B, C, H, W = tf.shape
            assert C == 3
        tp = tp.detach().to(torch.float32).contiguous()
        assert tuple(tp.shape) == (B, H, W)
        dev = tf.device
        packed = self._ensure_packed()
        lib, dt = L.lib(), _DTYPES[self.precision]
        nbytes = lib.ivosw_assess_ws_bytes(dt, B, H, W, self.chunk)
        ws = self._ws.get(nbytes, dev)
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        features = torch.empty(B, 2048, dtype=torch.float32, device=dev)
        fwd = lib.ivosw_assess_forward_features_u8 if u8 else lib.ivosw_assess_forward_features
        L.check(fwd(L.dptr(packed), dt, L.dptr(tf), L.dptr(tp), B, H, W, L.dptr(scores), L.dptr(features), L.dptr(ws), nbytes, self.chunk,
                    L.stream_ptr(dev)), "assess_forward_features_u8" if u8 else "assess_forward_features")
        return scores, features

    # ------------------------------------------------------------------ fitting the score head
    def fit_head(self, features, targets, valid, *, lr, momentum, weight_decay, gamma, num_epochs, batch_size, seed, zero_grad=True,
                 configs=None, holdout=None):
        """The reference's optimiser loop (quality_assessment.py: per-sample MSE over the rows with a non-empty union, backward,
        clamp_(-1, 1), SGD with momentum and weight decay, ExponentialLR per epoch) applied to fc1 on a bank of pooled features
        (``forward_features``) with the trunk frozen: ivosw_head_fit, every epoch of every config in one launch per 32 configs.

        features [M,2048] fp32, targets [M], valid [M] (bool / uint8) on the device.  ``holdout``: row indices (or a bool mask) kept out
        of the fit; one eval-only pass scores them per config afterwards.  ``configs``: a list of dicts overriding lr, momentum,
        weight_decay, gamma, zero_grad - a sweep; every config starts from the present fc1 and sees the same shuffles (numpy
        RandomState(seed): one permutation of the training rows per epoch, cut into full batches like DataLoader(shuffle=True,
        drop_last=True)).  zero_grad=False is the reference as written: it never calls zero_grad(), so the clamped gradients accumulate.
        Nothing is written to fc1 (``set_head`` does that).  One device-to-host copy, at the end."""
        dev = features.device
        features = features.detach().to(torch.float32).contiguous()
        M = int(features.shape[0])
        if features.dim() != 2 or features.shape[1] != 2048 or M < 1:
            raise ValueError(f"features must be [M,2048] with M >= 1, got {tuple(features.shape)}")
        targets = targets.detach().to(device=dev, dtype=torch.float32).contiguous().view(-1)
        valid = valid.detach().to(device=dev).ne(0).to(torch.uint8).contiguous().view(-1)
        if targets.numel() != M or valid.numel() != M:
            raise ValueError("targets and valid must hold one entry per feature row")
        base = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, gamma=gamma, zero_grad=zero_grad)
        cfgs = [dict(base)] if not configs else [dict(base, **c) for c in configs]
        for c in cfgs:
            extra = set(c) - set(base)
            if extra:
                raise ValueError(f"fit_head: unknown config keys {sorted(extra)} (a config may set {sorted(base)})")
        num_epochs, batch_size = int(num_epochs), int(batch_size)
        if num_epochs < 1:
            raise ValueError("num_epochs must be at least 1")
        if not 1 <= batch_size <= L.HEAD_FIT_MAX_BATCH:
            raise ValueError(f"batch_size must be 1 .. {L.HEAD_FIT_MAX_BATCH}, got {batch_size}")
        held = np.zeros(M, dtype=bool)
        if holdout is not None:
            h = holdout.detach().cpu().numpy() if isinstance(holdout, torch.Tensor) else np.asarray(holdout)
            if h.dtype == bool:
                if h.shape != (M,):
                    raise ValueError("a holdout mask must hold one entry per feature row")
                held = h.copy()
            else:
                if h.size and (h.min() < 0 or h.max() >= M):
                    raise ValueError("holdout index out of range")
                held[h.astype(np.int64)] = True
        train_rows, held_rows = np.flatnonzero(~held), np.flatnonzero(held)
        steps = len(train_rows) // batch_size
        if steps < 1:
            raise ValueError(f"fit_head: {len(train_rows)} training rows do not fill one batch of {batch_size} (drop_last)")
        rng = np.random.RandomState(int(seed))
        order = np.concatenate([train_rows[rng.permutation(len(train_rows))[:steps * batch_size]] for _ in range(num_epochs)])
        order = order.astype(np.int32).reshape(num_epochs * steps, batch_size)
        assert order.min() >= 0 and order.max() < M                       # the table the kernel trusts
        n_steps, n_cfg = num_epochs * steps, len(cfgs)
        lr_tab = np.stack([np.repeat(np.array([float(c["lr"]) * float(c["gamma"]) ** e for e in range(num_epochs)],
                                              dtype=np.float64).astype(np.float32), steps) for c in cfgs])
        # the held-out rows as full batches of one size: the largest divisor of their count that a launch takes
        hb = max([d for d in range(1, min(L.HEAD_FIT_MAX_BATCH, len(held_rows)) + 1) if len(held_rows) % d == 0], default=0)
        h_steps = len(held_rows) // hb if hb else 0
        lib, st = L.lib(), L.stream_ptr(dev)
        order_d = torch.from_numpy(order).to(dev)
        h_order_d = torch.from_numpy(held_rows.astype(np.int32)).to(dev) if hb else None
        lr_d = torch.from_numpy(lr_tab).to(dev)
        # everything the host wants back, in one flat tensor: w | b | log | held-out log
        n_w, n_log, n_hlog = n_cfg * 2048, n_cfg * n_steps * 3, n_cfg * h_steps * 3
        out = torch.zeros(n_w + n_cfg + n_log + n_hlog, dtype=torch.float32, device=dev)
        w = out[:n_w].view(n_cfg, 2048)
        b = out[n_w:n_w + n_cfg]
        log = out[n_w + n_cfg:n_w + n_cfg + n_log].view(n_cfg, n_steps, 3)
        hlog = out[n_w + n_cfg + n_log:].view(n_cfg, h_steps, 3)
        w.copy_(self.fc1.weight.detach().to(device=dev, dtype=torch.float32).view(1, 2048).expand(n_cfg, 2048))
        b.copy_(self.fc1.bias.detach().to(device=dev, dtype=torch.float32).view(1).expand(n_cfg))
        state_w = torch.zeros(2, n_cfg, 2048, dtype=torch.float32, device=dev)         # momentum buffers | gradient accumulators of w
        state_b = torch.zeros(2, n_cfg, dtype=torch.float32, device=dev)               # ... of b
        taken = torch.zeros(n_cfg, dtype=torch.int32, device=dev)
        f_arr, i_arr = (lambda v: (ctypes.c_float * len(v))(*v)), L.int_array
        for g in range(0, n_cfg, L.HEAD_FIT_MAX_FITS):
            grp = cfgs[g:g + L.HEAD_FIT_MAX_FITS]
            k = len(grp)
            mom, wd = f_arr([float(c["momentum"]) for c in grp]), f_arr([float(c["weight_decay"]) for c in grp])
            zg = i_arr([1 if c["zero_grad"] else 0 for c in grp])
            ptrs = [L.torch_ptr(out, g * 2048), L.torch_ptr(out, n_w + g), L.torch_ptr(state_w, g * 2048), L.torch_ptr(state_b, g),
                    L.torch_ptr(state_w, (n_cfg + g) * 2048), L.torch_ptr(state_b, n_cfg + g), L.torch_ptr(taken, g)]
            # (one index table serves the whole group: every fit of a launch reads its own [n_steps,B] slice, so the table is repeated)
            order_g = order_d.unsqueeze(0).expand(k, n_steps, batch_size).contiguous()
            L.check(lib.ivosw_head_fit(L.dptr(features), L.dptr(targets), L.dptr(valid), M, L.dptr(order_g), L.torch_ptr(lr_d, g * n_steps),
                                       k, n_steps, batch_size, mom, wd, zg, i_arr([0] * k), *ptrs, L.torch_ptr(out, n_w + n_cfg + g * n_steps * 3), st),
                    "head_fit")
            if hb:
                h_order_g = h_order_d.view(1, h_steps, hb).expand(k, h_steps, hb).contiguous()
                L.check(lib.ivosw_head_fit(L.dptr(features), L.dptr(targets), L.dptr(valid), M, L.dptr(h_order_g),
                                           L.torch_ptr(lr_d, g * n_steps), k, h_steps, hb, mom, wd, zg, i_arr([1] * k), *ptrs,
                                           L.torch_ptr(out, n_w + n_cfg + n_log + g * h_steps * 3), st), "head_fit (held-out rows)")
        host = out.cpu().numpy().astype(np.float64)                         # the one device-to-host copy
        w_h, b_h = host[:n_w].reshape(n_cfg, 2048), host[n_w:n_w + n_cfg]
        log_h = host[n_w + n_cfg:n_w + n_cfg + n_log].reshape(n_cfg, num_epochs, steps, 3)
        hlog_h = host[n_w + n_cfg + n_log:].reshape(n_cfg, h_steps, 3)
        took = np.maximum((log_h[..., 2] > 0).sum(2), 1)                    # the reference's meters average over the steps it took
        res = HeadFitResult()
        res.configs, res.steps_per_epoch, res.num_epochs, res.batch_size = cfgs, steps, num_epochs, batch_size
        res.log = log
        res.epoch_loss, res.epoch_diff = log_h[..., 0].sum(2) / took, log_h[..., 1].sum(2) / took
        res.w, res.b = torch.from_numpy(w_h.astype(np.float32)), torch.from_numpy(b_h.astype(np.float32))
        res.holdout_loss = res.holdout_diff = res.holdout_n = None
        if holdout is not None:
            n = hlog_h[..., 2].sum(1) if hb else np.zeros(n_cfg)
            d = np.maximum(n, 1)
            res.holdout_n = n.astype(np.int64)
            res.holdout_loss = (hlog_h[..., 0] * hlog_h[..., 2]).sum(1) / d if hb else np.zeros(n_cfg)
            res.holdout_diff = (hlog_h[..., 1] * hlog_h[..., 2]).sum(1) / d if hb else np.zeros(n_cfg)
        key = res.holdout_loss if (res.holdout_n is not None and res.holdout_n.min() > 0) else res.epoch_loss[:, -1]
        key = np.where(np.isfinite(key), key, np.inf)
        res.best = int(np.argmin(key))
        return res

    def set_head(self, w, b):
        """Write fc1 in place (w: 2048 values, b: one) and drop the packed copy: a later ``forward`` scores with this head.  Nothing else
        of the network changes."""
        w = torch.as_tensor(w).detach().reshape(-1)
        b = torch.as_tensor(b).detach().reshape(-1)
        if w.numel() != 2048 or b.numel() != 1:
            raise ValueError(f"set_head takes 2048 weights and one bias, got {w.numel()} and {b.numel()}")
        with torch.no_grad():
            self.fc1.weight.copy_(w.to(self.fc1.weight).view(1, 2048))
            self.fc1.bias.copy_(b.to(self.fc1.bias))
        self.invalidate_packed()

    def forward_tap(self, tf, tp, tap):
        """Debug/test hook: also returns one intermediate (NHWC; see ``_TAPS``)."""
        return self._run(tf, tp, tap)

    def all2yxhw(self, mask, scale=1.5):
        """Binary mask [B,H,W] -> (y,x,h,w) [B,4] on device (models/assessment.py:110-161)."""
        if scale != 1.5:
            raise ValueError("the HIP bbox kernel implements the scale=1.5 the reference forward uses")
        m = mask.detach().to(torch.float32).contiguous()
        B, H, W = m.shape
        out = torch.empty(B, 4, dtype=torch.float32, device=m.device)
        scratch = torch.empty(B, 4, dtype=torch.int32, device=m.device)
        L.check(L.lib().ivosw_mask_bbox(L.dptr(m), B, H, W, L.dptr(out), L.dptr(scratch), L.stream_ptr(m.device)),
                "mask_bbox")
        return out
