"""Golden-vector generator for the session overlays.  Runs ONLY where the reference tree is at hand: it imports the reference's
utils/utils_ipn.py on the CPU with ``cv2`` stubbed in sys.modules (none of the overlay functions calls it), runs overlay_davis,
overlay_fade, overlay_checker and overlay_color on small uint8 images and records inputs and outputs next to this file.  The fixture is
data; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_overlay_goldens.py <reference root>
"""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np

SIZES = ((9, 33), (33, 70))
N_OBJECTS = 3
PALETTE3 = ((128, 0, 0), (0, 128, 0), (128, 128, 0))       # objects 1 .. 3 of the DAVIS colour map
ABOVE = 200                                                # a label value above N_OBJECTS: no object


def case(H, W):
    """An image with every byte extreme in it and a label map of three objects that touch each other, all four borders and every
    corner, with two objects one pixel apart and label values above N_OBJECTS next to them."""
    rng = np.random.default_rng(100 * H + W)
    blocks = rng.integers(0, 256, ((H + 5) // 6, (W + 9) // 10, 3), dtype=np.uint8)       # 6 x 10 blocks of one colour: the fixture stays small
    image = np.ascontiguousarray(blocks.repeat(6, 0).repeat(10, 1)[:H, :W])
    image[H // 2, : W // 2] = 255
    image[H // 2, W // 2:] = 0
    image[0, 0], image[H - 1, W - 1] = (255, 254, 253), (1, 2, 3)
    lab = np.zeros((H, W), np.uint8)
    lab[: H // 2, : W // 3] = 1                            # the top-left corner
    lab[: H // 3, W // 3:] = 2                             # touches object 1 along a column; the top-right corner
    lab[H - 2:, :] = 3                                     # both bottom corners
    lab[H // 2: H - 2, :2] = 3                             # ... and up the left border until it touches object 1 from below
    lab[H // 3 + 1, W // 3 + 9] = 1                        # one pixel below object 2, one row of nothing between them
    lab[H // 3, W // 3] = ABOVE                            # in the corner between objects 1 and 2
    lab[H // 2 + 1, W // 2] = ABOVE
    lab[H // 2 + 1, W // 2 + 1] = N_OBJECTS + 1
    lab[H // 2, W - 1] = 2                                 # a single pixel on the right border
    spots = rng.random((H, W)) < 0.04
    spots[: H // 2 + 2] = False
    spots[H - 3:] = False
    lab[spots] = rng.integers(1, N_OBJECTS + 2, int(spots.sum()))
    return image, lab


def main():
    ref_root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IVOSW_REFERENCE", ""))
    assert os.path.isfile(os.path.join(ref_root, "utils", "utils_ipn.py")), "usage: make_overlay_goldens.py <reference root>"
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_root)
    os.chdir(HERE)
    warnings.simplefilter("ignore", DeprecationWarning)    # the reference imports scipy.ndimage.morphology
    from utils import utils_ipn as ref
    assert ref.__file__.startswith(ref_root), ref.__file__
    out = {"sizes": np.array(SIZES, np.int32), "palette3": np.array(PALETTE3, np.uint8), "n_objects": np.array(N_OBJECTS)}
    for H, W in SIZES:
        image, lab = case(H, W)
        key = f"{H}x{W}_"
        out[key + "image"], out[key + "label"] = image, lab
        keep = image.copy()
        for alpha in (0.5, 0.3):
            out[key + f"davis_a{alpha}"] = ref.overlay_davis(image, lab, alpha=alpha)                  # rgb = [255, 0, 0], mask == 1
            out[key + f"davis_rgb_a{alpha}"] = ref.overlay_davis(image, lab, rgb=[10, 201, 77], alpha=alpha)
            run = image
            for o in range(1, N_OBJECTS + 1):              # the sequential composition, ascending object order, on the running image
                run = ref.overlay_davis(run, lab == o, rgb=list(PALETTE3[o - 1]), alpha=alpha)
            out[key + f"davis_seq_a{alpha}"] = run
            out[key + f"davis_obj2_a{alpha}"] = ref.overlay_davis(image, lab == 2, rgb=list(PALETTE3[1]), alpha=alpha)
        out[key + "fade"] = ref.overlay_fade(image, lab)
        out[key + "checker"] = ref.overlay_checker(image, lab)
        out[key + "color"] = ref.overlay_color(image, lab)
        out[key + "color_rgb"] = ref.overlay_color(image, lab, rgb=[3, 250, 9])
        assert np.array_equal(keep, image)
        for k, v in out.items():
            assert v.dtype in (np.uint8, np.int32, np.int64), (k, v.dtype)
            assert not k.startswith(key) or k.endswith("label") or v.shape == (H, W, 3), (k, v.shape)
    path = os.path.join(HERE, "overlay_fixtures.npz")
    np.savez_compressed(path, **out)
    print("overlay_fixtures.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
