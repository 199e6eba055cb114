"""Golden-vector generator for rough_ROI.  Runs ONLY where the reference tree is at hand: it imports the reference's
utils/utils_manet.py on the CPU with ``davisinteractive`` and MANet's ``config`` stubbed in sys.modules (rough_ROI uses neither), runs
that ONE function on small label maps and records inputs and outputs next to this file.  The fixture is data; no reference source
travels.  (The function warns about its uint8 ``where`` condition under a current torch; the values are unaffected.)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scribble_goldens.py <reference root>
"""
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np

SMALL, LARGE = (30, 40), (120, 214)


def blank(b, size):
    return np.full((b, 1) + size, -1.0, np.float32)


def cases():
    """name -> float32 [b,1,h,w]: -1 everywhere but the scribbled pixels (values 0, 1, 2)."""
    out = {}
    for tag, (h, w) in (("s", SMALL), ("l", LARGE)):
        for name, (y, x) in dict(tl=(0, 0), tr=(0, w - 1), bl=(h - 1, 0), br=(h - 1, w - 1), mid=(h // 2, w // 2)).items():
            m = blank(1, (h, w))                           # one pixel in each corner and in the middle
            m[0, 0, y, x] = 1.0
            out[f"{tag}_pixel_{name}"] = m
        for name, (ys, xs) in dict(top=(slice(0, 3), slice(w // 3, w // 2)), bottom=(slice(h - 3, h), slice(w // 3, w // 2)),
                                   left=(slice(h // 3, h // 2), slice(0, 3)), right=(slice(h // 3, h // 2), slice(w - 3, w)),
                                   all=(slice(0, h), slice(0, w))).items():
            if tag == "l":                                 # (at the small size only: the fixture stays small)
                break
            m = blank(1, (h, w))                           # boxes that touch each border: the exclusive ends
            m[0, 0, ys, xs] = 2.0
            m[0, 0, ys, xs][::2, ::2] = 0.0
            out[f"{tag}_touch_{name}"] = m
    h, w = LARGE
    m = blank(1, LARGE)                                    # farther than 20 from every border
    m[0, 0, 50:61, 100:111] = 1.0
    out["l_far"] = m
    m = blank(1, LARGE)                                    # closer than 20 to the top and the left, exactly 20 and 21 away elsewhere
    m[0, 0, 5:h - 21, 8:w - 22] = 1.0
    m[0, 0, 30:60, 40:90] = -1.0                           # -1 inside the box stays -1
    out["l_near"] = m
    m = blank(1, LARGE)
    m[0, 0, 20, 20] = 0.0                                  # a background scribble exactly 20 from the top-left corner
    m[0, 0, h - 21, w - 21] = 2.0                          # hmax + 20 == h - 1
    out["l_exact20"] = m
    rng = np.random.default_rng(20)
    for tag, size in (("s", SMALL), ("l", LARGE)):
        m = blank(2, size)                                 # b = 2 with different boxes, values 0, 1, 2 and -1 inside them
        hh, ww = size
        for i, (ys, xs) in enumerate(((slice(2, hh // 2), slice(3, ww // 3)), (slice(hh // 2, hh - 1), slice(ww // 2, ww)))):
            sub = np.where(rng.random((ys.stop - ys.start, xs.stop - xs.start)) < 0.2, rng.integers(0, 3, (ys.stop - ys.start, xs.stop - xs.start)), -1)
            sub[0, 0], sub[-1, -1] = 1, 2
            m[i, 0, ys, xs] = sub
        out[f"{tag}_batch2"] = m
    return out


def main():
    ref_root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IVOSW_REFERENCE", ""))
    assert os.path.isfile(os.path.join(ref_root, "utils", "utils_manet.py")), "usage: make_scribble_goldens.py <reference root>"
    import torch
    for name in ("davisinteractive", "davisinteractive.dataset", "davisinteractive.dataset.davis", "config"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["davisinteractive.dataset.davis"].Davis = object
    sys.modules["config"].cfg = object()
    sys.path.insert(0, ref_root)
    os.chdir(HERE)
    from utils import utils_manet as ref
    assert ref.__file__.startswith(ref_root), ref.__file__
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # where() with a uint8 condition
        for name, m in cases().items():
            keep = m.copy()
            got = ref.rough_ROI(torch.from_numpy(m)).numpy()
            assert np.array_equal(keep, m) and got.shape == m.shape and got.dtype == np.float32
            out["in_" + name] = m.astype(np.int8)          # the inputs hold -1, 0, 1, 2 only: stored as bytes
            out["out_" + name] = got.astype(np.int8)
            assert np.array_equal(out["out_" + name].astype(np.float32), got)
    path = os.path.join(HERE, "scribble_fixtures.npz")
    np.savez_compressed(path, **out)
    print("scribble_fixtures.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
