"""Golden-vector generator for the IPN glue.  Runs ONLY in the build container: it imports the reference's utils/utils_ipn.py
(/root/reference, read-only) with ``cv2`` stubbed in sys.modules, the way make_goldens.py stubs its imports (Dilate_mask, the one
function that calls cv2, is not recorded), and records the reference's own answers next to this file.  The fixture is data; no
reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ipn_goldens.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np
import torch

# (target, prev_targets, num_frames, at_least)
WEIGHT_CASES = [
    (5, [], 12, -1),                 # no neighbour
    (5, [], 12, 4),
    (5, [9], 12, -1),                # a neighbour on the right only
    (5, [2], 12, -1),                # ... on the left only
    (5, [2, 9], 12, -1),             # both sides
    (5, [0, 2, 9, 11], 12, -1),      # the nearest one on each side decides
    (5, [4, 6], 12, -1),             # adjacent frames
    (5, [4, 6], 12, 3),              # at_least biting on both sides
    (5, [3, 9], 12, 3),              # biting on the left only
    (5, [1, 10], 12, 3),             # not biting
    (1, [0, 3], 12, 4),              # biting, and clipped at frame 0
    (10, [8, 11], 12, 5),            # biting, and clipped at the last frame
    (0, [], 7, -1),                  # target at frame 0
    (0, [4], 7, -1),
    (0, [1], 7, 3),
    (6, [], 7, -1),                  # target at the last frame
    (6, [3], 7, -1),
    (6, [5], 7, 3),
    (3, [0, 6], 7, -1),              # thirds and sixths: weights that do not round-trip through float32
    (50, [20, 93], 100, 7),
]


def label_cases():
    rng = np.random.default_rng(2017)
    out = []
    for K, T, H, W, index in ((2, 2, 3, 4, [1, 0]), (3, 2, 3, 5, [2, 0, 1]), (4, 1, 2, 3, [1, 3, 0, 2]), (4, 3, 2, 2, [0, 1, 2, 3]),
                              (1, 2, 2, 2, [0])):
        E = rng.random((1, K, T, H, W), dtype=np.float32)
        if K > 1:
            E[0, 1, 0, 0, :2] = E[0, 0, 0, 0, :2]        # exact ties between positions 0 and 1: the lower CANONICAL channel wins
            E[0, :, -1, -1, -1] = 0.25                   # every channel ties
            E[0, 0, 0, 1, 0], E[0, 1, 0, 1, 0] = 0.0, -0.0
            E[0, 2:, 0, 1, 0] = -1.0
        out.append((K, index, E))
    return out


def main():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, REF)
    os.chdir("/tmp")
    from utils import utils_ipn as ref
    assert ref.__file__.startswith(REF), ref.__file__
    out = {"get_weight": [], "to_np_label": []}
    for target, prev, n, at_least in WEIGHT_CASES:
        left, right, weight = ref.Get_weight(target, list(prev), n, at_least)
        out["get_weight"].append(dict(target=target, prev_targets=prev, num_frames=n, at_least=at_least, left_end=int(left),
                                      right_end=int(right), weight=[float(w) for w in weight]))      # json round-trips Python floats
    for K, index, E in label_cases():
        lab = ref.To_np_label(torch.from_numpy(E), K, list(index))
        assert lab.dtype == np.uint8
        out["to_np_label"].append(dict(K=K, index=index, shape=list(E.shape), E_bits=E.view(np.uint32).reshape(-1).tolist(),
                                       label=lab.reshape(-1).tolist(), label_shape=list(lab.shape)))
    with open(os.path.join(HERE, "ipn_fixtures.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("ipn_fixtures.json", len(out["get_weight"]), "weight cases,", len(out["to_np_label"]), "label cases,",
          os.path.getsize(os.path.join(HERE, "ipn_fixtures.json")), "bytes")


if __name__ == "__main__":
    main()
