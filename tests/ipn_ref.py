"""Host references of the IPN glue (csrc/ipn_glue.hip) in numpy, exact: the dilation as the reference's literal per-object loop
(scipy's binary_dilation standing in for cv2's, which is not a dependency) and as the diamond maximum of include/ivosw.h, the three-step
fp32 blend, and the labels as a literal restatement of To_np_label.  tests/test_ipn_option.py pins them against each other and against
the recorded fixtures; the GPU tests share them."""
import numpy as np

try:
    from scipy import ndimage
except ImportError:                                    # dilate_ref then falls back to the diamond maximum; the scipy asserts are skipped
    ndimage = None

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)          # cv2.getStructuringElement(cv2.MORPH_CROSS, (3, 3))


def dilate_diamond(mask, num_objects):
    """The rule of include/ivosw.h on [..., H, W]: the largest o in 0 .. num_objects within |dy| + |dx| <= 2 inside the image, else -1;
    values outside -1 .. num_objects count as -1."""
    mask = np.asarray(mask).astype(np.int64)
    m = np.where((mask >= 0) & (mask <= num_objects), mask, -1)
    H, W = m.shape[-2:]
    pad = np.full(m.shape[:-2] + (H + 4, W + 4), -1, np.int64)
    pad[..., 2:-2, 2:-2] = m
    out = np.full(m.shape, -1, np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(dy) + abs(dx) <= 2:
                out = np.maximum(out, pad[..., 2 + dy:2 + dy + H, 2 + dx:2 + dx + W])
    return out


def dilate_ref(mask, num_objects):
    """Dilate_mask (utils/utils_ipn.py:26-34) on one [H, W] map, literally: per object a binary dilation of (mask == o) with the 3x3
    cross, 2 iterations, overwriting in ascending object order."""
    mask = np.asarray(mask)
    if ndimage is None:
        return dilate_diamond(mask, num_objects)
    new_mask = -np.ones_like(mask, dtype=np.int64)
    for o in range(num_objects + 1):
        dmask = ndimage.binary_dilation(mask == o, structure=CROSS, iterations=2)
        new_mask[np.where(dmask == 1)] = o
    return new_mask


def weights32(weight):
    """(float32(w), float32(1 - float64(w))) per frame: what torch makes of the Python scalars w and 1 - w against a float32 tensor."""
    w = np.asarray(weight, dtype=np.float64)
    return w.astype(np.float32), (1 - w).astype(np.float32)


def blend32(new, old, weight):
    """new, old [K, T, ...] float32, weight [T]: (w * new) + ((1 - w) * old) per frame as three separately rounded float32
    operations (no FMA), on every frame."""
    wn, wo = weights32(weight)
    new, old = np.asarray(new, dtype=np.float32), np.asarray(old, dtype=np.float32)
    shape = (1, -1) + (1,) * (new.ndim - 2)
    m1 = (wn.reshape(shape) * new).astype(np.float32)
    m2 = (wo.reshape(shape) * old).astype(np.float32)
    return (m1 + m2).astype(np.float32)


def canonical(E, index):
    """E [K, ...] with index[j] = the canonical channel held at position j -> the channels in canonical order."""
    inv_index = [list(index).index(i) for i in range(len(index))]
    return np.asarray(E)[inv_index]


def labels_ref(E, index):
    """To_np_label (utils/utils_ipn.py:75-81) on E [K, T, H, W] without the batch axis, literally.  numpy's argmax defines the corner
    cases: the first maximum wins, a NaN is the maximum and the first NaN wins, -0.0 and 0.0 tie."""
    K = len(index)
    sh_E = np.asarray(E)
    inv_index = [list(index).index(i) for i in range(K)]
    E = sh_E[inv_index]
    fgs = np.argmax(E, axis=0)
    return fgs.astype(np.uint8)
