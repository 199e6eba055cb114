"""Pins the references and the inputs of tests/test_gpu_front_multi_edges.py on the CPU (oracle/front_ref.py): the chunk rule of a
launch over a video table, the one-hot planes and the dirty units of a label map, and - before any kernel meets them - that the
lone-pixel positions and the byte values of the GPU test tell three deliberately wrong scans from the right one: a carried (y, x)
that forgets the row wrap, a scan that drops the last vector of a chunk, a byte test that also takes label ^ 0x80 or label + 1."""
import numpy as np
import pytest

from oracle import front_ref as fr

BIG = np.iinfo(np.int32).max

# (label scan?, H, W, rows of the launch, strides inside a chunk?) - the scans of the GPU test, with the chunk each one runs at
SCANS = [(False, 480, 854, 32, False), (False, 70, 1100, 32, True), (False, 80, 1024, 32, True)] + \
        [(False, H, W, 2049, True) for H, W in fr.ONE_CHUNK_SIZES] + \
        [(True, 480, 854, 32, True), (True, 480, 854, 128, True)] + [(True, H, W, 2049, True) for H, W in fr.LABEL_ONE_CHUNK_SIZES]
CHUNKS = {(False, 480, 854): 7168, (False, 70, 1100): 2048, (False, 80, 1024): 2048, (False, 4, 1025): 5120, (False, 4, 1024): 4096,
          (False, 4, 1100): 5120, (False, 2048, 2): 4096, (False, 8, 8): 1024, (True, 480, 854, 32): 7168, (True, 480, 854, 128): 26624,
          (True, 16, 1100): 18432, (True, 16, 1024): 16384}


def test_scan_seams_multi_rule():
    plane = 480 * 854
    chunk, (seams,) = fr.scan_seams_multi([plane], 1)                              # S = 64: ceil(409920 / 64) = 6405 -> 7168, 58 chunks
    assert chunk == 7168 and len(seams) == 57 and seams[0] == 7168 and seams[-1] == 57 * 7168
    assert fr.scan_seams_multi([plane], 32)[0] == 7168 and fr.scan_seams_multi([plane], 33)[0] == 7168          # S = 64, 62: 6612 -> 7168
    chunk, (seams,) = fr.scan_seams_multi([plane], 128)                            # S = 16: 25620 -> 26624, 16 chunks
    assert chunk == 26624 and len(seams) == 15
    chunk, (seams,) = fr.scan_seams_multi([plane], 2049)                           # S = 1: the whole plane, rounded up
    assert chunk == 410624 and seams == []
    # a table: the chunk comes from the largest plane, a smaller plane is cut at the same chunk or not at all
    chunk, seams = fr.scan_seams_multi([plane, 70 * 1100, 37 * 53, 4], 42)         # S = 48: 8540 -> 9216
    assert chunk == 9216 and len(seams[0]) == 44 and seams[1] == list(range(9216, 77000, 9216)) and seams[2] == [] and seams[3] == []
    assert fr.scan_seams_multi([4, 4100, 4096], 4000) == (5120, [[], [], []])


@pytest.mark.parametrize("B", [1, 7, 33, 40, 128, 2048, 2049])
def test_scan_seams_multi_is_scan_seams_on_one_plane(B):
    for H, W in fr.BBOX_SIZES + fr.MULTI_CARRY_SIZES + fr.ONE_CHUNK_SIZES:
        chunk, (seams,) = fr.scan_seams_multi([H * W], B)
        assert seams == fr.scan_seams(B, H, W) and chunk % 1024 == 0


def test_stride_edges_keeps_its_float_positions_and_takes_the_label_stride():
    assert fr.stride_edges(3, 1100) == sorted({0, 1099, 2200, 3299, 3296, 1023, 1024, 1027, 2047, 2048, 2051, 3071, 3072, 3075})
    assert fr.stride_edges(16, 1100, 4096, 16) == sorted({0, 1099, 16500, 17599, 17584} | {s + d for s in (4096, 8192, 12288, 16384)
                                                                                         for d in (-1, 0, 15)})


def test_label_planes_and_label_delta_ref_by_hand():
    rs = np.random.RandomState(4)
    lab = rs.randint(0, 6, (3, 5, 7)).astype(np.uint8)                             # 0 .. 5 with n_obj = 4: 5 belongs to nobody
    planes = fr.label_planes(lab, 4)
    assert planes.dtype == np.float32 and planes.shape == (12, 5, 7)
    for obj in range(4):
        for f in range(3):
            for y in range(5):
                for x in range(7):
                    assert planes[obj * 3 + f, y, x] == (1.0 if lab[f, y, x] == obj + 1 else 0.0)
    new = lab.copy()
    assert fr.label_delta_ref(lab, new, 4) == []
    lab[1, 2, 3], new[1, 2, 3] = 2, 4                                              # 2 -> 4 in frame 1: units (1, 1) and (1, 3)
    assert fr.label_delta_ref(lab, new, 4) == [1 * 3 + 1, 3 * 3 + 1]
    lab[0, 0, 0], new[0, 0, 0] = 0, 5                                              # 0 <-> n_obj + 1: nothing
    lab[2, 4, 6], new[2, 4, 6] = 5, 0
    assert fr.label_delta_ref(lab, new, 4) == [4, 10]
    lab[2, 0, 0], new[2, 0, 0] = 0, 1                                              # 0 -> 1 in frame 2; 3 -> 200 in frame 0
    lab[0, 4, 0], new[0, 4, 0] = 3, 200
    assert fr.label_delta_ref(lab, new, 4) == [2, 4, 6, 10]
    # the definition: the units whose one-hot planes differ
    a, b = fr.label_planes(lab, 4), fr.label_planes(new, 4)
    assert fr.label_delta_ref(lab, new, 4) == [u for u in range(12) if (a[u] != b[u]).any()]
    assert fr.label_delta_ref(lab, new, 2) == [2, 4]                               # n_obj = 2: labels 3 and 4 belong to nobody


def _lone_boxes(H, W, pos):
    """bbox_minmax_ref of the lone-pixel planes, from the planes themselves."""
    out = np.empty((len(pos), 4), np.int32)
    for k in range(0, len(pos), 16):
        out[k:k + 16] = fr.bbox_minmax_ref(fr.lone_planes(H, W, pos[k:k + 16]))
    return out


def _walk_boxes(H, W, pos, chunk, label, **wrong):
    stride, vec = (4096, 16) if label else (1024, 4)
    out = np.empty((len(pos), 4), np.int32)
    for k, p in enumerate(pos):
        yx = fr.scan_walk(p, H, W, chunk, stride, vec, **wrong)
        out[k] = (BIG, -1, BIG, -1) if yx is None else (yx[0], yx[0], yx[1], yx[1])
    return out


@pytest.mark.parametrize("label,H,W,B,strides", SCANS)
def test_lone_pixels_tell_a_wrong_carry_and_a_dropped_vector(label, H, W, B, strides):
    """The positions of the GPU test at the chunk the launch really uses: every seam has a lone pixel on each side, every stride inside
    a chunk too (where the case asks for them), and the plane's last vector; the kernel's walk, restated, gives the reference on all of
    them; the walk WITHOUT the row wrap of the carried step and the scan WITHOUT the last vector of a chunk each give another box."""
    stride, vec = (4096, 16) if label else (1024, 4)
    chunk, pos = fr.lone_positions(H, W, B, label, strides)
    plane = H * W
    assert chunk == CHUNKS[(label, H, W, B) if (label and W == 854) else (label, H, W)]
    _, (seams,) = fr.scan_seams_multi([plane], B)
    assert all(s - 1 in pos and s in pos for s in seams) and {0, plane - 1, max(0, plane - vec)} <= set(pos)
    inner = [s for beg in range(0, plane, chunk) for s in range(beg + stride, min(plane, beg + chunk), stride)]
    if strides:
        assert all(s - 1 in pos and s in pos and min(plane - 1, s + vec - 1) in pos for s in inner)
        assert (len(inner) > 0) == (min(plane, chunk) > stride)
    want = _lone_boxes(H, W, pos)
    np.testing.assert_array_equal(want, np.array([[p // W, p // W, p % W, p % W] for p in pos], np.int32))
    np.testing.assert_array_equal(_walk_boxes(H, W, pos, chunk, label), want)     # the restated walk is the kernel's right one
    carried = min(plane, chunk) > stride
    no_wrap = _walk_boxes(H, W, pos, chunk, label, wrap=False)
    if carried and stride % W != 0:
        assert (no_wrap != want).any(axis=1).sum() >= 2, "a forgotten row wrap passes on these positions"
    else:                                                                          # nothing carried, or sx = 0 (W = 1024, W = 2): no wrap to forget
        np.testing.assert_array_equal(no_wrap, want)
    dropped = _walk_boxes(H, W, pos, chunk, label, drop_last=True)
    lost = {pos[k] for k in np.flatnonzero((dropped != want).any(axis=1))}
    assert {s - 1 for s in seams} | {plane - 1} <= lost and not ({0} | set(seams)) & lost - {plane - 1}


def test_hard_byte_map_tells_a_sloppy_byte_test():
    """On every unit of hard_byte_units the one-hot plane is the label's own two bytes; a test that also takes label ^ 0x80, or
    label + 1, or label - 1, gives another integer box on every one of them - at n_obj = 255 and at n_obj = 100, where the values above
    100 belong to no unit."""
    m = fr.hard_byte_map()
    assert m.shape == (5, 16, 256) and m.dtype == np.uint8 and m.max() == 255
    for n_obj in (255, 100):
        right = fr.bbox_minmax_ref(fr.label_planes(m, n_obj))
        units = [(lab - 1) * 5 + f for f, lab in fr.hard_byte_units(n_obj)]
        assert len(units) == n_obj
        for f, lab in fr.hard_byte_units(n_obj):
            at = 16 * lab + 4 * ((lab >> 1) & 1)
            np.testing.assert_array_equal(right[(lab - 1) * 5 + f], [at // 256, at // 256, at % 256 + 1, at % 256 + 4])
        for other in (lambda v: v ^ 0x80, lambda v: (v + 1) & 255, lambda v: (v - 1) & 255):
            wrong = np.concatenate([((m == o + 1) | (m == other(o + 1))).astype(np.float32) for o in range(n_obj)], 0)
            assert (fr.bbox_minmax_ref(wrong)[units] != right[units]).any(axis=1).all()
    # every label sits next to its neighbours inside ONE 32-bit word, and one word holds the neighbours without it
    for lab in (1, 2, 127, 128, 129, 200, 254, 255):
        w = fr.hard_bytes(lab).reshape(3, 4)
        assert lab in w[0] and lab in w[1] and lab not in w[2]
        assert {lab ^ 0x80, (lab - 1) & 255, (lab + 1) & 255} <= set(w[0].tolist()) and {0, 255} <= set(w[1].tolist()) | {lab}
