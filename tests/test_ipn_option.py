"""CPU: the host side of the IPN glue - Get_weight and To_np_label's restatement against what the reference itself answered
(tests/golden/ipn_fixtures.json, recorded by tests/golden/make_ipn_goldens.py), the numpy references the GPU tests share
(tests/ipn_ref.py) against each other, the two C declarations against their bindings and the build list, the argument refusals of the
entries (made before any pointer is used: fake pointers, no GPU) and the refusals of the host wrappers."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd.utils import utils_ipn as ui
from tests import ipn_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "ipn_fixtures.json")))


# ---------------------------------------------------------------------------------------------- Get_weight, weights32
def test_get_weight_is_the_references():
    kinds = set()
    for c in FIX["get_weight"]:
        prev = list(c["prev_targets"])
        left, right, weight = ui.Get_weight(c["target"], prev, c["num_frames"], c["at_least"])
        assert (left, right) == (c["left_end"], c["right_end"]), c
        assert weight == c["weight"] and all(type(w) is float for w in weight), c          # Python floats, equal bit for bit
        assert prev == c["prev_targets"] and weight[c["target"]] == 1.0
        kinds.add((any(p < c["target"] for p in prev), any(p > c["target"] for p in prev), c["at_least"] > 0))
    assert len(kinds) == 8                                # every combination of left / right neighbour and at_least
    assert ui.Get_weight(5, [2, 9], 12)[2][3:8] == [1.0 - 2 * (1.0 / 3), 1.0 - 1.0 / 3, 1.0, 0.75, 0.5]


def test_weights32_is_torchs_scalar_rule():
    for c in FIX["get_weight"]:
        wn, wo = ui.weights32(c["weight"])
        rn, ro = ir.weights32(c["weight"])
        assert wn.dtype == wo.dtype == np.float32 and wn.flags.c_contiguous and wo.flags.c_contiguous
        np.testing.assert_array_equal(wn.view(np.uint32), rn.view(np.uint32))
        np.testing.assert_array_equal(wo.view(np.uint32), ro.view(np.uint32))
    # against torch itself: (w * new) + ((1 - w) * old) with Python scalars, frame by frame
    rng = np.random.default_rng(9)
    new, old = rng.random((3, 7, 4, 5), dtype=np.float32), rng.random((3, 7, 4, 5), dtype=np.float32)
    weight = ui.Get_weight(3, [0, 6], 7)[2]
    assert any(float(np.float32(w)) != w for w in weight)                                  # thirds: they do not round-trip
    want = np.stack([((w * torch.from_numpy(new[:, f])) + ((1 - w) * torch.from_numpy(old[:, f]))).numpy() for f, w in enumerate(weight)], 1)
    got = ir.blend32(new, old, weight)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... which an FMA would not reproduce, and neither would float32(1) - float32(w)
    wn, wo = ir.weights32(weight)
    fused = (wn[None, :, None, None].astype(np.float64) * new + (wo[None, :, None, None] * old).astype(np.float32)).astype(np.float32)
    assert (fused != got).any()
    w3 = np.float64(1.0 / 3.0)
    assert np.float32(1 - w3) != np.float32(1) - np.float32(w3) and ui.weights32([1.0 / 3.0])[1][0] == np.float32(1 - w3)


# ---------------------------------------------------------------------------------------------- the numpy references
def test_labels_ref_is_the_references_to_np_label():
    for c in FIX["to_np_label"]:
        E = np.array(c["E_bits"], dtype=np.uint32).view(np.float32).reshape(c["shape"])
        got = ir.labels_ref(E[0], c["index"])
        assert got.dtype == np.uint8 and list(got.shape) == c["label_shape"]
        np.testing.assert_array_equal(got.reshape(-1), np.array(c["label"], dtype=np.uint8))
        np.testing.assert_array_equal(got, np.argmax(ir.canonical(E[0], c["index"]), axis=0))
    assert any(c["index"] != sorted(c["index"]) for c in FIX["to_np_label"])
    # the corner cases the kernel must follow: first maximum, -0.0 ties 0.0, a NaN is the maximum and the first NaN wins
    E = np.array([[0.5, -0.0, 1.0, np.nan, 2.0], [0.5, 0.0, np.nan, np.nan, 1.0], [0.5, -0.0, np.nan, 3.0, 2.0]], np.float32).reshape(3, 1, 1, 5)
    np.testing.assert_array_equal(ir.labels_ref(E, [0, 1, 2]).reshape(-1), [0, 0, 1, 0, 0])
    np.testing.assert_array_equal(ir.labels_ref(E, [2, 1, 0]).reshape(-1), [0, 0, 0, 1, 0])   # canonical 0 sits at position 2


def test_dilate_ref_is_the_diamond_maximum():
    rng = np.random.default_rng(4)
    for H, W in ((1, 1), (1, 6), (2, 7), (5, 5), (9, 33), (17, 70)):
        for num_objects in (0, 1, 3):
            m = np.where(rng.random((H, W)) < 0.12, rng.integers(0, num_objects + 3, (H, W)), -1)        # values above num_objects too
            m[0, 0], m[-1, -1], m[0, -1], m[-1, 0] = 0, num_objects, 0, num_objects
            want = ir.dilate_diamond(m, num_objects)
            assert want.dtype == np.int64 and want.min() >= -1 and want.max() <= num_objects
            if ir.ndimage is not None:
                np.testing.assert_array_equal(ir.dilate_ref(m, num_objects), want, err_msg=f"{H}x{W}, {num_objects}")
    one = -np.ones((7, 9), np.int64)
    one[3, 4] = 1
    want = np.where(np.abs(np.arange(7)[:, None] - 3) + np.abs(np.arange(9)[None] - 4) <= 2, 1, -1)
    np.testing.assert_array_equal(ir.dilate_diamond(one, 1), want)
    np.testing.assert_array_equal(ir.dilate_diamond(one, 0), -np.ones((7, 9), np.int64))   # object 1 is out of range for num_objects = 0
    np.testing.assert_array_equal(ir.dilate_ref(one, 1), want)


# ---------------------------------------------------------------------------------------------- C ABI
def _declaration(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivosw.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    d = flat[flat.index(f"int {name}("):]
    return [p.strip() for p in d[d.index("(") + 1:d.index(");")].split(",")]


def test_header_binding_and_build_list_agree():
    kinds = {"int": L._i, "float": L._f, "long": ctypes.c_long}
    names = {"ivosw_ipn_dilate": ["mask", "n", "H", "W", "num_objects", "out", "stream"],
             "ivosw_ipn_merge": ["all_E", "prev_E", "K", "T", "H", "W", "w_new32", "w_old32", "index", "probs", "probs_stride_c", "label_u8",
                                 "label_f32", "stream"]}
    for name, want_names in names.items():
        params = _declaration(name)
        want = [L._p if ("*" in p or p.startswith("ivosw_stream_t")) else kinds[p.split()[0]] for p in params]
        res, args = L.SIGNATURES[name]
        assert res is L._i and args == want, params
        assert [p.split()[-1].lstrip("*") for p in params] == want_names
    assert "IPN glue (8f-4, IPN)" in open(os.path.join(ROOT, "include", "ivosw.h")).read()
    spec = importlib.util.spec_from_file_location("ivosw_build_for_test", os.path.join(ROOT, "ivos-w_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "ipn_glue.hip" in b.SOURCES and os.path.exists(os.path.join(b.CSRC, "ipn_glue.hip"))
    src = open(os.path.join(b.CSRC, "ipn_glue.hip")).read()
    assert "IVOSW_IPN_SCALAR" in src and "fp contract(off)" in src
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "utils_ipn" in text and "ipn_merge" in text, doc
    for doc in ("README.md", os.path.join("include", "ivosw.h"), os.path.join("ivos-w_amd", "utils", "utils_ipn.py")):
        assert "unpinned" in open(os.path.join(ROOT, doc)).read().split("model.Run", 1)[1], doc


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_entries_refuse_before_any_pointer_is_used(lib):
    """Host pointers that must never be dereferenced as device memory: every case is refused by the argument checks, which come before
    the device lookup."""
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    P, Q = ctypes.c_void_p(base), ctypes.c_void_p(base + 2048)
    msg = lambda: lib.ivosw_last_error().decode()

    def dilate(mask=P, n=2, H=6, W=8, num_objects=3, out=Q):
        return lib.ivosw_ipn_dilate(mask, n, H, W, num_objects, out, None)

    for kw, text in [(dict(mask=None), "null mask"), (dict(out=None), "null out"), (dict(n=0), "bad shape"), (dict(H=0), "bad shape"),
                     (dict(W=-1), "bad shape"), (dict(num_objects=-1), "[0, 126]"), (dict(num_objects=127), "[0, 126]"),
                     (dict(H=65536, W=32768), "too large"), (dict(out=P), "must not be mask")]:
        assert dilate(**kw) == -1 and text in msg() and "ivosw_ipn_dilate" in msg(), (kw, msg())
    for kw in (dict(), dict(num_objects=126), dict(num_objects=0), dict(H=32768, W=65535)):
        assert dilate(**kw) == -1 and "not a device pointer" in msg(), (kw, msg())

    wn = (ctypes.c_float * 300)(*([0.5] * 300))
    perm = lambda *v: (ctypes.c_int * len(v))(*v)

    def merge(E=P, prev=Q, K=3, T=2, H=4, W=4, wn=wn, wo=wn, index=None, probs=None, sc=32, u8=Q, f32=None):
        return lib.ivosw_ipn_merge(E, prev, K, T, H, W, wn, wo, index, probs, sc, u8, f32, None)

    far = ctypes.c_void_p(base + 1024)                    # 3 * 2 * 16 floats = 384 bytes: [base, base + 384) and [base + 1024, ..) are apart
    cases = [(dict(E=None), "null all_E"), (dict(K=0), "[1, 32]"), (dict(K=33), "[1, 32]"), (dict(T=0), "bad shape"), (dict(H=0), "bad shape"),
             (dict(W=0), "bad shape"), (dict(H=65536, W=32768), "too large"), (dict(K=32, T=1 << 20, H=1 << 10, W=1 << 6), "2^40"),
             (dict(index=perm(0, 1, 1)), "not a permutation"), (dict(index=perm(0, 1, 3)), "not a permutation"),
             (dict(index=perm(-1, 1, 2)), "not a permutation"), (dict(wn=None), "needs w_new32"), (dict(wo=None), "needs w_new32"),
             (dict(probs=P), "overlaps all_E"), (dict(probs=ctypes.c_void_p(base + 380)), "overlaps all_E"),
             (dict(E=far, probs=ctypes.c_void_p(base + 1024 - 4 * (2 * 32 + 32) + 4)), "overlaps all_E"),
             (dict(probs=far, sc=31), "channels overlap"), (dict(probs=far, sc=1 << 40), "too large"),
             (dict(prev=None, u8=None), "no output"), (dict(prev=None, wn=None, wo=None, u8=None, f32=None, probs=None), "no output")]
    for kw, text in cases:
        assert merge(**kw) == -1 and text in msg() and "ivosw_ipn_merge" in msg(), (kw, msg())
    # what passes the argument checks ends at the device lookup (these are host pointers): still refused, with another message
    for kw in (dict(), dict(prev=None, wn=None, wo=None), dict(index=perm(2, 0, 1), probs=far), dict(K=1, probs=far, sc=0),
               dict(K=32, T=1 << 19, H=1 << 10, W=1 << 6), dict(E=far, probs=ctypes.c_void_p(base + 1024 - 4 * (2 * 32 + 32))),
               dict(probs=ctypes.c_void_p(base + 384)), dict(prev=None, u8=None, f32=Q)):
        assert merge(**kw) == -1 and "not a device pointer" in msg(), (kw, msg())
    assert 32 * (1 << 19) * (1 << 16) == 1 << 40


def test_new_kernels_have_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    table = kr.kernel_table(L.LIB_PATH)
    for key in ("ipn_dilate_kernel", "ipn_merge_kernel"):
        hits = [r for n, r in table.items() if key in n]
        assert len(hits) == 2 and all(r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 for r in hits), (key, hits)


# ---------------------------------------------------------------------------------------------- the host wrappers' own checks
def test_the_wrappers_refuse_before_touching_a_device():
    K, T, H, W = 3, 4, 6, 8
    store = ui.IpnStore(T, K, H, W, "cpu")
    assert store.buf is store.all_E and tuple(store.buf.shape) == (K, T, H, W) and store.all_P.shape == (T, K, H, W)
    assert store.labels_u8.dtype == torch.uint8 and store.final_masks.dtype == torch.float32 and store.final_masks.shape == (T, H, W)
    mine = torch.rand(1, K, T, H, W)
    wrapped = ui.IpnStore(T, K, H, W, "cpu", all_E=mine)
    assert wrapped.all_E.data_ptr() == mine.data_ptr() and wrapped.all_P.data_ptr() == mine.data_ptr()
    assert torch.equal(wrapped.all_P, mine[0].transpose(0, 1))
    label_only = ui.IpnStore(T, K, H, W, "cpu", probs=False)
    assert label_only.buf is None and label_only.all_E is None and label_only.all_P.map is label_only.labels_u8
    with pytest.raises(ValueError, match="positive"):
        ui.IpnStore(0, K, H, W, "cpu")
    with pytest.raises(ValueError, match="at most 32"):
        ui.IpnStore(T, 33, H, W, "cpu")
    with pytest.raises(ValueError, match="estimate must be"):
        ui.IpnStore(T, K, H, W, "cpu", all_E=torch.zeros(K, T + 1, H, W))

    E, prev, w = torch.rand(1, K, T, H, W), torch.rand(1, K, T, H, W), [1.0, 0.5, 0.25, 0.0]
    with pytest.raises(TypeError, match="IpnStore"):
        ui.merge_round(E, prev, w, None, object())
    with pytest.raises(TypeError, match="float32"):
        ui.merge_round(E.double(), prev, w, None, store)
    with pytest.raises(TypeError, match="float32"):
        ui.merge_round(E, prev.half(), w, None, store)
    with pytest.raises(TypeError, match="float32"):
        ui.merge_round(E.numpy(), prev, w, None, store)
    with pytest.raises(ValueError, match="estimate must be"):
        ui.merge_round(E[:, :2], prev, w, None, store)
    with pytest.raises(ValueError, match="estimate must be"):
        ui.merge_round(torch.rand(2, K, T, H, W), prev, w, None, store)
    with pytest.raises(ValueError, match="contiguous"):
        ui.merge_round(torch.rand(1, K, T, W, H).transpose(3, 4), prev, w, None, store)
    with pytest.raises(ValueError, match="weights for 4 frames"):
        ui.merge_round(E, prev, w[:3], None, store)
    for bad in ([0, 1], [0, 1, 1], [1, 2, 3], [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="not a permutation"):
            ui.merge_round(E, prev, w, bad, store)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # everything fits: only the device is missing
        ui.merge_round(E, prev, w, [2, 0, 1], store)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ui.merge_round(E, None, None, None, store)
    assert store.own is None and store.buf is store.all_E             # nothing was bound or allocated on the way

    with pytest.raises(TypeError, match="float32"):
        ui.To_np_label(E.double(), K, [0, 1, 2])
    with pytest.raises(ValueError, match="channels"):
        ui.To_np_label(E, K + 1, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="not a permutation"):
        ui.To_np_label(E, K, [0, 2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ui.To_np_label(E, K, [1, 0, 2])

    m = torch.full((2, H, W), -1, dtype=torch.int8)
    with pytest.raises(TypeError, match="int8"):
        ui.dilate_scribbles(m.long(), 2)
    with pytest.raises(ValueError, match=r"\[n,H,W\]"):
        ui.dilate_scribbles(m[None], 2)
    with pytest.raises(ValueError, match="outside"):
        ui.dilate_scribbles(m, 127)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ui.dilate_scribbles(m, 2)
    with pytest.raises(ValueError, match="integer"):
        ui.Dilate_mask(np.zeros((H, W), np.float32), 2)
    with pytest.raises(ValueError, match="integer"):
        ui.Dilate_mask(np.zeros((2, H, W), np.int64), 2)
    with pytest.raises(ValueError, match="outside"):
        ui.Dilate_mask(np.zeros((H, W), np.int64), -1)


def test_to_cuda_helpers_keep_the_references_results():
    mask = np.array([[1, 0, -1], [2, 1, 0]])
    P, N = ui.ToCudaPN(mask)
    assert P.shape == N.shape == (1, 2, 3) and P.dtype == N.dtype == torch.float32 and not P.requires_grad
    np.testing.assert_array_equal(P.cpu().numpy()[0], (mask == 1).astype(np.float32))
    np.testing.assert_array_equal(N.cpu().numpy()[0], (mask == 0).astype(np.float32))
    a, b = ui.ToCudaVariable([torch.ones(2), torch.zeros(3)], requires_grad=True)
    assert a.requires_grad and b.requires_grad and a.is_leaf and a.is_cuda == torch.cuda.is_available()
