"""The overlay kernel (ivosw_overlay_frames) against the host sequence it replaces, at 480p (480 x 854), a session of 100 frames with 1
and 3 objects, frames held as RGBX8 bytes and as fp32 planes, the four styles (GPU only).

  device    utils_ipn.overlay_session - ONE ivosw_overlay_frames call on the frames and the label map that sit on the device - plus the
            ONE copy that brings the pictures to the host.
  host      what a caller did before: the label maps and the frames of the wanted frames copied to the host (packed frames: their
            bytes; float frames: the planes, turned into bytes there), then the reference's functions restated on the host - per object
            a float64 blend of the whole image and scipy.ndimage.binary_dilation for the contour (tests/overlay_ref.py where scipy is
            not importable), the objects in sequence for davis.
  Both render the 4 candidate frames, alternating, host clock around work that ends in a synchronise: medians and min .. max over 5
  rounds.  All 100 frames: the device leg the same way; the host leg is timed ONCE per condition (it takes seconds).
  kernel    the call alone, all 100 frames, per kernel path - W = 854 (the width of DAVIS 480p: 2 pixels per lane), the same forced to
            the scalar kernel, and W = 856 (4 pixels per lane), the path asked of the library for the very buffers used: HIP events
            around 10 calls, per call; the bytes it moves (counted from the shapes: 4 or 12 B of frame, 1 B of label and 3 or 4 B of
            picture per pixel) over its time, against the 6.3 TB/s float4 copy figure.

usage: python tools/overlay_probe.py [--out profiles/overlay_probe.txt]      (the report goes to stdout and to that file)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, H, W, T, COPY_TBS = 5, 480, 854, 100, 6.3
CANDIDATES = [12, 40, 41, 87]
STYLES = ("davis", "fade", "checker", "color")


def _events(fn, n, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / n                # us per call


def _wall(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3             # ms


def _fmt(v, unit):
    return f"{statistics.median(v):9.3f} {unit} ({min(v):.3f} .. {max(v):.3f})"


def host_overlay(image, label, style, n_objects, palette):
    """The reference's functions restated with scipy: one picture from a uint8 [H,W,3] image and its label map, every object drawn."""
    import numpy as np
    try:
        from scipy.ndimage import binary_dilation
    except ImportError:
        from tests import overlay_ref
        return overlay_ref.overlay_one(image, label, style, n_objects)
    if style == "davis":
        out = image
        for o in range(1, n_objects + 1):
            m = label == o
            fg = out * 0.5 + np.ones(out.shape) * (1 - 0.5) * palette[o - 1][None, None, :]
            out = out.copy()
            out[m] = fg[m]
            out[binary_dilation(m) ^ m, :] = 0
        return out
    m = (label >= 1) & (label <= n_objects)
    if style == "fade":
        out = image.copy()
        out[~m] = 0.4 * out[~m]
        out[binary_dilation(m) ^ m] = (0, 255, 255)
        return out
    if style == "checker":
        yy, xx = np.mgrid[:image.shape[0], :image.shape[1]]
        board = np.where((yy // 20 + xx // 20) % 2 == 0, 223, 32).astype(np.uint8)[..., None].repeat(3, 2)
    else:
        board = np.ones(image.shape, dtype=np.uint8) * np.array((255, 0, 255), dtype=np.uint8)[None, None, :]
    board[m] = image[m]
    return board


def kernel_paths(say, dev):
    """The call alone, all T frames, 3 objects, per kernel path: W = 854 (DAVIS 480p: 2 pixels per lane), the same forced to the scalar
    kernel, and W = 856 (4 pixels per lane).  The path is asked of the library (ivosw_overlay_lane_pixels) for the very buffers used."""
    import numpy as np
    import torch
    from ivos_w_amd import _lib as L
    from ivos_w_amd.models.assessment import PackedFrames
    from ivos_w_amd.utils import utils_ipn as ui
    say(f"kernel alone, {T} frames, 3 objects, HIP events around 10 calls, per call; bytes counted from the shapes (4 or 12 B of frame, 1 B of "
        f"label, 3 or 4 B of picture per pixel) against the {COPY_TBS} TB/s float4 copy figure")
    for width, scalar in ((W, False), (W, True), (W + 2, False)):
        rng = np.random.default_rng(width)
        packed = PackedFrames(torch.from_numpy(rng.integers(0, 256, (T, H, width, 4), dtype=np.uint8)).to(dev))
        planes = packed.to_float()
        lab_t = torch.from_numpy(rng.integers(0, 4, (T, H // 16, width // 8), dtype=np.uint8).repeat(16, 1).repeat(8 + (width % 8 > 0), 2)
                                 [:, :, :width].copy()).to(dev)
        if scalar:
            os.environ["IVOSW_OVERLAY_SCALAR"] = "1"    # read by the launcher at every call
        for kind, frames in (("RGBX8", packed), ("F32", planes)):
            for out in ("rgb", "rgbx"):
                sample = ui.overlay_session(frames, lab_t, 3, out=out)
                lanes = L.lib().ivosw_overlay_lane_pixels(L.dptr(frames.rgbx if kind == "RGBX8" else frames), L.dptr(lab_t), width,
                                                          L.dptr(sample), L.OUT_RGBX8 if out == "rgbx" else L.OUT_RGB8)
                del sample
                for style in STYLES:
                    k = [_events(lambda: ui.overlay_session(frames, lab_t, 3, style=style, out=out), 10, dev) for _ in range(ROUNDS)]
                    moved = T * H * width * ((4 if kind == "RGBX8" else 12) + 1 + (4 if out == "rgbx" else 3))
                    us = statistics.median(k)
                    say(f"W = {width}{' forced scalar' if scalar else '':14s} {lanes} px/lane  {kind:5s} -> {out:4s} {style:8s} {_fmt(k, 'us')}  "
                        f"{moved / 1e6:.0f} MB -> {moved / us / 1e6:.2f} TB/s, {100 * moved / us / 1e6 / COPY_TBS:.0f} %")
        os.environ.pop("IVOSW_OVERLAY_SCALAR", None)
        del packed, planes, lab_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_probe.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from ivos_w_amd.models.assessment import PackedFrames
    from ivos_w_amd.utils import utils_ipn as ui
    from tests import overlay_ref
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"overlay probe: {H} x {W}, {T} frames, candidates {CANDIDATES}, {ROUNDS} rounds, medians (min .. max)")
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    packed = PackedFrames(torch.from_numpy(np.concatenate([u8, np.zeros((T, H, W, 1), np.uint8)], 3)).to(dev))
    planes = packed.to_float()
    palette = ui.davis_palette()
    yy, xx = np.mgrid[:H, :W]
    for n_objects in (1, 3):
        lab = np.zeros((T, H, W), np.uint8)
        for f in range(T):                              # n_objects discs that drift, the second and third touching
            for o in range(n_objects):
                cy, cx = 240 + 60 * o + f // 2, 250 + 150 * o + f
                lab[f][(yy - cy) ** 2 + (xx - cx) ** 2 < 90 ** 2] = o + 1
        lab_t = torch.from_numpy(lab).to(dev)
        for kind, frames in (("RGBX8", packed), ("F32", planes)):
            for style in STYLES:
                keep = {}

                def device(ids):
                    keep["dev"] = ui.overlay_session(frames, lab_t, n_objects, style=style, frame_ids=ids).cpu().numpy()

                def host(ids):
                    sel = torch.as_tensor(list(range(T)) if ids is None else ids, device=dev)
                    lab_h = lab_t[sel].cpu().numpy()
                    if kind == "RGBX8":
                        img = packed.rgbx[sel].cpu().numpy()[..., :3]
                    else:
                        img = overlay_ref.frame_bytes(planes[sel].cpu().numpy())
                    keep["host"] = np.stack([host_overlay(img[j], lab_h[j], style, n_objects, palette) for j in range(len(lab_h))])

                device(CANDIDATES), host(CANDIDATES)
                same = bool(np.array_equal(keep["dev"], keep["host"]))
                r = {"device": [], "host": []}
                for _ in range(ROUNDS):
                    r["device"].append(_wall(lambda: device(CANDIDATES), dev))
                    r["host"].append(_wall(lambda: host(CANDIDATES), dev))
                ratio = statistics.median(r["host"]) / statistics.median(r["device"])
                say(f"{style:8s} {kind:5s} {n_objects} obj   4 candidates: device {_fmt(r['device'], 'ms')}   host {_fmt(r['host'], 'ms')}   "
                    f"x{ratio:.0f}   pictures equal: {same}")
                device(None)
                d_all = [_wall(lambda: device(None), dev) for _ in range(ROUNDS)]
                h_all = _wall(lambda: host(None), dev)
                say(f"{'':22s} all {T} frames: device {_fmt(d_all, 'ms')}   host {h_all:9.1f} ms (once)   x{h_all / statistics.median(d_all):.0f}")
                del keep
        del lab_t
    del packed, planes
    kernel_paths(say, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
