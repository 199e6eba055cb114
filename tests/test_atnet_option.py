"""CPU: the host side of the ATNet epilogue - the blend weight, the numpy reference the GPU tests share (tests/atnet_ref.py) against
a literal restatement with torch CPU ops, the C declaration against its binding and the build list, the argument refusals of the
entry (made before any pointer is used: fake pointers, no GPU) and the shape checks of the glue."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd.utils import utils_atnet as ua
from tests import atnet_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------- prop_alpha
def test_prop_alpha_hand_computed_cases():
    # no earlier / later annotated frame in the direction of travel: 1
    assert ua.prop_alpha([6], 6, 3, 1) == 1 and ua.prop_alpha([6], 6, 9, 2) == 1
    assert ua.prop_alpha([8, 6], 6, 3, 1) == 1            # the other annotation lies ahead: backward is unblended
    assert ua.prop_alpha([2, 6], 6, 9, 2) == 1            # ... and behind: forward is unblended
    # backward from 6 towards an annotation at 2: midway 0.75, at the other annotation 0.5, one step from it 0.5 + 0.5 / 4
    assert ua.prop_alpha([2, 6], 6, 4, 1) == 0.75
    assert ua.prop_alpha([2, 6], 6, 2, 1) == 0.5
    assert ua.prop_alpha([2, 6], 6, 3, 1) == 0.625
    assert ua.prop_alpha([2, 6], 6, 5, 1) == 0.875
    # forward from 6 towards an annotation at 10, the mirror image
    assert ua.prop_alpha([10, 6], 6, 8, 2) == 0.75
    assert ua.prop_alpha([10, 6], 6, 10, 2) == 0.5
    assert ua.prop_alpha([10, 6], 6, 9, 2) == 0.625
    # the CLOSEST annotation in the direction decides; a gap of 3: adjacent to the other annotation 0.5 + 0.5 / 3 in float64
    assert ua.prop_alpha([0, 3, 9, 6], 6, 4, 1) == 0.5 + 0.5 * ((4 - 3) / (6 - 3))
    assert ua.prop_alpha([0, 3, 9, 6], 6, 8, 2) == 0.5 + 0.5 * ((9 - 8) / (9 - 6))
    assert isinstance(float(ua.prop_alpha([0, 3, 9, 6], 6, 8, 2)), float)


# ---------------------------------------------------------------------------------------------- the numpy reference
def test_reference_matches_a_literal_torch_restatement():
    rng = np.random.default_rng(5)
    n_obj, PH, PW = 3, 11, 13
    x = (rng.standard_normal((n_obj, PH, PW)) * 6).astype(np.float32)
    x[0, 0, :4] = (0.0, -0.0, 104.0, -104.0)
    old = rng.random((n_obj, PH, PW), dtype=np.float32)
    # float64 sigmoid: torch's, to a few float64 ulps; exact at 0; finite and in [0, 1] at the extremes
    s64 = ar.sigmoid64(x)
    t64 = torch.sigmoid(torch.from_numpy(x).double()).numpy()
    assert np.abs(s64 - t64).max() <= 4 * 2.0 ** -53 and s64[0, 0, 0] == 0.5 and s64[0, 0, 1] == 0.5
    assert np.isfinite(s64).all() and s64.min() >= 0 and s64.max() <= 1 and 0 < s64[0, 0, 3] < ar.FLT_MIN
    # the blend: three separately rounded float32 operations, torch's scalar handling included
    s32 = torch.sigmoid(torch.from_numpy(x))
    for alpha in (1, 0.5, 0.75, 0.5 + 0.5 / 3, 0.5 + 0.5 * (2 / 7)):
        want = ((alpha * s32) + ((1 - alpha) * torch.from_numpy(old))).numpy()
        got = ar.blend32(s32.numpy(), old, alpha)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(alpha))
    # ... which an FMA would NOT reproduce: the reference is sensitive to what it pins
    a32, b32 = ar.alpha_beta32(0.5 + 0.5 / 3)
    fused = (np.float64(a32) * s32.numpy().astype(np.float64) + (b32 * old).astype(np.float32).astype(np.float64)).astype(np.float32)
    assert (fused != ar.blend32(s32.numpy(), old, 0.5 + 0.5 / 3)).any()
    # the label rule: first maximum, strict threshold
    p = ar.blend32(s32.numpy(), old, 0.75)
    p[1, 2] = p[0, 2]                                     # ties between objects 0 and 1 on a row
    p[2, 2] = 0.0
    p[:, 3, :5] = 0.5
    for th in (0.5, 0.8, np.nextafter(np.float32(0.5), np.float32(0))):
        tp = torch.from_numpy(p)
        am = tp.argmax(0)                                 # torch: "the indices of the first maximal value"
        best = tp.gather(0, am[None])[0]
        want = torch.where(best > float(np.float32(th)), am + 1, torch.zeros_like(am)).numpy()
        got = ar.labels(p, th)
        np.testing.assert_array_equal(got, want)
        assert (got[2] <= 1).all()
    assert (ar.labels(p, 0.5)[3, :5] == 0).all() and (ar.labels(p, np.nextafter(np.float32(0.5), np.float32(0)))[3, :5] == 1).all()
    assert ar.crop(p, (1, 2, 3, 4)).shape == (n_obj, PH - 3, PW - 7)


# ---------------------------------------------------------------------------------------------- C ABI
def _declaration():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivosw.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    d = flat[flat.index("int ivosw_atnet_epilogue("):]
    return d[:d.index(");")]


def test_header_binding_and_build_list_agree():
    d = _declaration()
    params = [p.strip() for p in d[d.index("(") + 1:].split(",")]
    kinds = {"int": L._i, "float": L._f, "long": ctypes.c_long}
    want = [L._p if ("*" in p or p.startswith("ivosw_stream_t")) else kinds[p.split()[0]] for p in params]
    res, args = L.SIGNATURES["ivosw_atnet_epilogue"]
    assert res is L._i and args == want, params
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "logits", "prob_map_t", "n_obj", "PH", "PW", "hpad1", "wpad1", "H", "W", "blend", "alpha32", "beta32", "th", "prob_pad", "probs",
        "probs_stride_c", "label_u8", "label_f32", "stream"]
    spec = importlib.util.spec_from_file_location("ivosw_build_for_test", os.path.join(ROOT, "ivos-w_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "atnet_epilogue.hip" in b.SOURCES and os.path.exists(os.path.join(b.CSRC, "atnet_epilogue.hip"))
    src = open(os.path.join(b.CSRC, "atnet_epilogue.hip")).read()
    assert "IVOSW_ATNET_SCALAR" in src and "fp contract(off)" in src
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "atnet_epilogue" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.fixture(scope="module")
def lib():
    if not L.available():
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_entry_refuses_before_any_pointer_is_used(lib):
    """Host pointers that must never be dereferenced: every case is refused by the argument checks, which come before the device lookup."""
    buf = ctypes.create_string_buffer(96)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    msg = lambda: lib.ivosw_last_error().decode()

    def call(logits=P, pm=P, n_obj=2, PH=20, PW=36, hpad1=2, wpad1=4, H=16, W=28, blend=0, prob_pad=P, probs=P, sc=16 * 28, u8=P, f32=P):
        return lib.ivosw_atnet_epilogue(logits, pm, n_obj, PH, PW, hpad1, wpad1, H, W, blend, 1.0, 0.0, 0.5, prob_pad, probs, sc, u8, f32, None)

    cases = [(dict(pm=None), "null prob_map_t"), (dict(n_obj=0), "n_obj < 1"), (dict(n_obj=256), "n_obj <= 255"), (dict(H=0), "bad shape"),
             (dict(W=0), "bad shape"), (dict(hpad1=-1), "negative pad"), (dict(wpad1=-1), "negative pad"), (dict(hpad1=5), "outside the padded grid"),
             (dict(wpad1=9), "outside the padded grid"), (dict(sc=16 * 28 - 1), "overlap"), (dict(PH=65536, PW=32768), "too large"),
             (dict(n_obj=3, PH=32768, PW=32768), "too large"), (dict(logits=None, blend=1), "blend needs logits"), (dict(blend=2), "0 or 1"),
             (dict(logits=None, probs=None, u8=None, f32=None), "no output")]
    for kw, text in cases:
        assert call(**kw) == -1 and text in msg() and "ivosw_atnet_epilogue" in msg(), (kw, msg())
    # what passes the argument checks ends at the device lookup (these are host pointers): still refused, with another message
    for kw in (dict(n_obj=256, u8=None), dict(n_obj=1, sc=0), dict(n_obj=1, PH=32768, PW=65535), dict(logits=None, prob_pad=None)):
        assert call(**kw) == -1 and "not a device pointer" in msg(), (kw, msg())
    assert (32768 * 65535) <= INT_MAX < 65536 * 32768 and 3 * 32768 * 32768 > INT_MAX


def test_new_kernels_have_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools on this host")
    hits = [r for n, r in kr.kernel_table(L.LIB_PATH).items() if "atnet_epilogue_kernel" in n]
    assert len(hits) == 3 and all(r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 for r in hits), hits


# ---------------------------------------------------------------------------------------------- the glue's own checks
def test_wrong_shapes_and_zero_trailing_pads_raise():
    n, n_obj, h, w = 3, 2, 6, 8
    pads = (1, 1, 2, 2)
    store = ua.AtnetStore(n, n_obj, h, w, "cpu")
    assert store.buf.shape == (n_obj + 1, n, h, w) and (store.buf[0] == 0).all() and store.all_P.shape == (n, n_obj + 1, h, w)
    assert store.labels_u8.dtype == torch.uint8 and store.final_masks.dtype == torch.float32
    label_only = ua.AtnetStore(n, n_obj, h, w, "cpu", probs=False)
    assert label_only.buf is None and label_only.all_P.map is label_only.labels_u8
    pm = torch.zeros(n, n_obj, h + 2, w + 4)
    x = torch.zeros(n_obj, 1, h + 2, w + 4)
    for bad in ((1, 0, 2, 2), (1, 1, 2, 0), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="EMPTY"):
            ua.atnet_epilogue(x, pm, 0, bad, 0.5, store)
        with pytest.raises(ValueError, match="EMPTY"):
            ua.run_VOS_singleiact(None, None, "val", {}, [0], np.zeros((n, h, w)), n, n_obj, 1, None, None, [], [], pm, *bad)
    with pytest.raises(ValueError, match="negative"):
        ua.atnet_epilogue(x, pm, 0, (-1, 1, 2, 2), 0.5, store)
    with pytest.raises(ValueError, match="plus the pads"):
        ua.atnet_epilogue(x, pm, 0, (1, 1, 2, 1), 0.5, store)
    with pytest.raises(ValueError, match="outside"):
        ua.atnet_epilogue(x, pm, n, pads, 0.5, store)
    with pytest.raises(ValueError, match="logits are not"):
        ua.atnet_epilogue(x[:1], pm, 0, pads, 0.5, store)
    with pytest.raises(ValueError, match="contiguous float32"):
        ua.atnet_epilogue(x, pm.double(), 0, pads, 0.5, store)
    with pytest.raises(ValueError, match="contiguous float32"):
        ua.atnet_epilogue(x, pm.permute(0, 1, 3, 2), 0, pads, 0.5, store)
    with pytest.raises(ValueError, match="does not match"):
        ua.atnet_epilogue(x, pm, 0, pads, 0.5, ua.AtnetStore(n + 1, n_obj, h, w, "cpu"))
    with pytest.raises(ValueError, match="probability buffer"):
        ua.atnet_epilogue(x, pm, 0, pads, 0.5, ua.AtnetStore(n, n_obj + 1, h, w, "cpu"))
    with pytest.raises(ValueError, match="needs logits"):
        ua.atnet_epilogue(None, pm, 0, pads, 0.5, store, alpha=0.5)
    with pytest.raises(ValueError, match="positive"):
        ua.AtnetStore(0, n_obj, h, w, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # everything fits: only the device is missing
        ua.atnet_epilogue(x, pm, 0, pads, 0.5, store)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.atnet_epilogue(None, pm, 0, pads, 0.5, store)
