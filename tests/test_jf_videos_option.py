"""CPU: the definition the device reduce (ivosw_jf_reduce_ragged) is held to - a pure-Python restatement of the J / F ratios, the row
mean and the J&F blend against the host path bit for bit - the ``metric`` config key, the Python grouping, and the new C declarations
against their bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivos_w_amd  # noqa: F401
from ivos_w_amd import _lib as L
from ivos_w_amd import entry, metrics
from ivos_w_amd.utils import utils_agent
from tests import jf_videos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the reduce rule
@pytest.mark.parametrize("n_obj", R.OBJECT_COUNTS)
def test_restated_reduce_rule_is_the_host_path_bit_for_bit(n_obj):
    counts = R.make_counts(R.min_frames(n_obj) + 3, n_obj, seed=n_obj)
    flat = [tuple(int(x) for x in c) for c in counts.reshape(-1, 6)]
    assert all(s in flat for s in R.SPECIAL)                             # every branch is in: empty union, the four precision / recall
    assert counts.max() > 2 ** 53 and np.ascontiguousarray(counts) is counts     # branches, p + r == 0, counts above 2^31 (and 2^53)
    for metric in R.METRICS:
        for average in (True, False):
            want = R.host_metric(counts, metric, average)
            got = R.restated(counts, metric, average)
            assert want.dtype == np.float64 and want.flags.c_contiguous and got.shape == want.shape
            np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64), err_msg=f"{metric} O={n_obj} average={average}")
            assert np.ptp(want) > 0


def test_the_row_mean_changes_its_order_at_eight_objects():
    # 1 + 2^-53 * k patterns: a sequential sum and numpy's 8-lane sum round differently, so the rule's order is observable
    rng = np.random.default_rng(0)
    seen = 0
    for n in (8, 9, 16, 17, 32):
        for _ in range(50):
            v = (rng.random(n) * 2.0 ** rng.integers(-20, 2, n)).astype(np.float64)
            want = v.reshape(1, n).mean(axis=1)[0]
            assert R.row_mean(list(v)) == want
            seq = v[0]
            for x in v[1:]:
                seq = seq + x
            seen += (seq / n) != want
    assert seen > 0
    for n in (1, 2, 3, 7):
        v = rng.random(n)
        assert R.row_mean(list(v)) == v.reshape(1, n).mean(axis=1)[0]


def test_f_from_evaluation_order_matters():
    # 2 * p * r / (p + r) in Python's order, not 2 * (p * r) / (p + r) reassociated differently or an FMA: the restatement keeps the order
    c = np.array([[[1, 3, 3, 7, 1, 2]]], dtype=np.int64)
    p, r = 1 / 3.0, 2 / 7.0
    assert metrics._f_from(c)[0, 0] == 2 * p * r / (p + r) == R.f_one(c[0, 0])


# ---------------------------------------------------------------------------------------------- config key
class AD(dict):
    __getattr__ = dict.__getitem__


def test_metric_key_parses_and_refuses_unknown_values():
    assert entry.DEFAULTS["metric"] == "host" and utils_agent.METRIC_MODES == ("host", "device")
    assert entry.parse_cli([]).metric == "host"
    assert entry.parse_cli(["with", "metric=device"]).metric == "device"
    assert entry.metric_option(entry.parse_cli(["with", "metric=device", "setting=oracle"])) == "device"
    assert utils_agent.metric_option(AD()) == "host" and utils_agent.metric_option(None) == "host"
    for bad in ("gpu", "Device", "1", "true", ""):
        with pytest.raises(SystemExit) as e:
            entry.parse_cli(["with", f"metric={bad}"])
        assert "metric must be 'host' or 'device'" in str(e.value)
    for bad in (1, True, None, "both"):
        with pytest.raises(ValueError, match="metric must be"):
            utils_agent.metric_option(AD(metric=bad))
    assert isinstance(utils_agent.ORACLE_MIN_SESSIONS, int) and utils_agent.ORACLE_MIN_SESSIONS >= 1


def test_oracle_recommend_refuses_other_settings_before_touching_anything():
    for setting, method in (("wild", "ours"), ("oracle", "random"), ("oracle", "linspace")):
        with pytest.raises(NotImplementedError):
            utils_agent.oracle_recommend(AD(setting=setting, method=method), None, "cpu", [dict()])
    assert utils_agent.oracle_recommend(AD(setting="oracle", method="worst"), None, "cpu", []) == ([], [])
    with pytest.raises(ValueError, match="davis_interactive.metric"):
        utils_agent.oracle_recommend(AD(setting="oracle", method="worst"), None, "cpu", [dict()])


# ---------------------------------------------------------------------------------------------- grouping
def test_groups_respect_the_table_size_and_both_grid_limits():
    G = metrics._jf_groups
    assert G([(1, 1)] * 70) == [(0, 32), (32, 64), (64, 70)]
    assert G([(3, 2)]) == [(0, 1)]
    assert G([(100, 32)] * 21) == [(0, 20), (20, 21)]                      # 3200 pairs a video: 20 fit 65535, the 21st does not
    assert G([(2100, 1)] * 32) == [(0, 31), (31, 32)]                      # 2100 frames a video: 31 fit
    assert G([(65535, 1), (1, 1)]) == [(0, 1), (1, 2)]
    for shapes in ([(2100, 1)] * 40, [(100, 32)] * 50, [(1, 1)] * 5 + [(30000, 2)] * 3 + [(7, 3)] * 40):
        groups = G(shapes)
        assert groups[0][0] == 0 and groups[-1][1] == len(shapes) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
        for a, b in groups:
            assert 0 < b - a <= L.MAX_JF_VIDEOS
            assert sum(n for n, _ in shapes[a:b]) <= metrics.GRID_LIMIT and sum(n * o for n, o in shapes[a:b]) <= metrics.GRID_LIMIT
    with pytest.raises(ValueError, match="video 1"):
        G([(5, 1), (65536, 1)])
    with pytest.raises(ValueError, match="video 0"):
        G([(3000, 32)])
    with pytest.raises(ValueError, match="metric must be one of"):
        metrics.jf_videos([], "JF")


# ---------------------------------------------------------------------------------------------- C ABI
def _declaration(name, res="int"):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivosw.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    d = flat[flat.index(f"{res} {name}("):]
    return [p.strip() for p in d[d.index("(") + 1:d.index(");")].split(",")]


def test_header_bindings_and_documents_agree():
    kinds = {"int": L._i, "size_t": L._sz}
    names = {"ivosw_jf_videos_ws_bytes": ("size_t", ["videos", "n_videos"]),
             "ivosw_jf_counts_videos": ("int", ["videos", "n_videos", "counts", "ws", "ws_bytes", "stream"]),
             "ivosw_jf_reduce_ragged": ("int", ["counts", "n_obj", "lengths", "n_seqs", "metric", "annot_counts", "per_obj", "quality", "state",
                                                "stream"])}
    for name, (res, want_names) in names.items():
        params = _declaration(name, res)
        want = [L._p if ("*" in p or p.startswith("ivosw_stream_t")) else kinds[p.split()[0]] for p in params]
        got_res, args = L.SIGNATURES[name]
        assert got_res is kinds[res] and args == want, params
        assert [p.split()[-1].lstrip("*") for p in params] == want_names
    hdr = open(os.path.join(ROOT, "include", "ivosw.h")).read()
    assert f"#define IVOSW_MAX_JF_VIDEOS {L.MAX_JF_VIDEOS}\n" in hdr and 1 <= L.MAX_JF_VIDEOS <= 32
    for k, v in (("J", L.METRIC_J), ("F", L.METRIC_F), ("J_AND_F", L.METRIC_J_AND_F)):
        assert f"#define IVOSW_METRIC_{k} {v}\n" in hdr and metrics.METRIC_CODES[k] == v
    # the ctypes mirror of ivosw_jf_video_t: two pointers, four ints, 32 ids, bound_pix - and a table of them fits the argument budget
    fields = [f[0] for f in L.JfVideo._fields_]
    assert fields == ["gt", "pred", "n_frames", "H", "W", "n_obj", "obj_ids", "bound_pix"]
    struct = hdr[hdr.index("typedef struct ivosw_jf_video {"):hdr.index("} ivosw_jf_video_t;")]
    assert [struct.index(f) for f in ("gt;", "pred;", "n_frames", "H,", "W,", "n_obj;", "obj_ids[32]", "bound_pix")] == \
        sorted(struct.index(f) for f in ("gt;", "pred;", "n_frames", "H,", "W,", "n_obj;", "obj_ids[32]", "bound_pix"))
    assert ctypes.sizeof(L.JfVideo) == 72 and L.JfVideo.obj_ids.offset == 32 and L.JfVideo.bound_pix.offset == 64
    src = open(os.path.join(ROOT, "ivos-w_amd", "csrc", "metrics.hip")).read()
    assert "fp contract(off)" in src and "sizeof(JfTable) <=" in src
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ivosw_jf_counts_videos" in text and "ivosw_jf_reduce_ragged" in text and "oracle_recommend" in text, doc
    assert "metric=device" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "jf_videos_probe.txt")) and os.path.exists(os.path.join(ROOT, "tools", "jf_videos_probe.py"))


def test_refusals_that_need_no_device():
    """Every check that comes before a pointer is used, with fake pointers: the code, the video's index in the message."""
    if not L.available():
        import __graft_entry__ as g
        g.build()
    lib = L.lib()
    msg = lambda: lib.ivosw_last_error().decode()
    fake = ctypes.c_void_p(4096)

    def table(*vs):
        out = []
        for kw in vs:
            d = dict(gt=4096, pred=8192, n_frames=2, H=5, W=7, n_obj=2, bound_pix=1)
            d.update(kw)
            out.append(L.JfVideo(**d))
        return (L.JfVideo * len(out))(*out), len(out)

    good = {}
    for bad, text in ((dict(gt=None), "NULL"), (dict(pred=None), "NULL"), (dict(n_frames=0), "positive"), (dict(H=0), "positive"),
                      (dict(W=-1), "positive"), (dict(n_obj=0), "1..32"), (dict(n_obj=33), "1..32"), (dict(bound_pix=-1), "0..32"),
                      (dict(bound_pix=33), "0..32")):
        t, n = table(good, bad, good)
        assert lib.ivosw_jf_counts_videos(t, n, fake, fake, 1 << 30, None) == -1 and "video 1:" in msg() and text in msg(), (bad, msg())
        assert lib.ivosw_jf_videos_ws_bytes(t, n) == 0
    t, n = table(good)
    assert lib.ivosw_jf_counts_videos(None, 1, fake, fake, 1 << 30, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_jf_counts_videos(t, 1, None, fake, 1 << 30, None) == -1 and "null pointer" in msg()
    assert lib.ivosw_jf_counts_videos(t, 1, fake, None, 1 << 30, None) == -1 and "null pointer" in msg()
    for n_bad in (0, -1, L.MAX_JF_VIDEOS + 1):
        big, _ = table(*([good] * (L.MAX_JF_VIDEOS + 1)))
        assert lib.ivosw_jf_counts_videos(big, n_bad, fake, fake, 1 << 30, None) == -1 and "n_videos" in msg()
    t, n = table(good, dict(n_frames=40000, n_obj=1), dict(n_frames=30000, n_obj=1))
    assert lib.ivosw_jf_counts_videos(t, n, fake, fake, 1 << 40, None) == -1 and "video 2:" in msg() and "frames in total" in msg()
    t, n = table(good, dict(n_frames=3000, n_obj=32))
    assert lib.ivosw_jf_counts_videos(t, n, fake, fake, 1 << 40, None) == -1 and "video 1:" in msg() and "(frame, object) pairs" in msg()
    # the workspace of a table is the sum of the single-video sizes
    t, n = table(good, dict(H=33, W=1025, n_obj=3), dict(n_frames=1, W=1))
    assert lib.ivosw_jf_videos_ws_bytes(t, n) == sum(lib.ivosw_jf_ws_bytes(v.n_frames, v.H, v.W, v.n_obj) for v in t) > 0

    ints = L.int_array
    args = lambda **kw: [kw.get(k, d) for k, d in (("counts", fake), ("n_obj", ints([2, 3])), ("lengths", ints([4, 5])), ("n_seqs", 2), ("metric", 2),
                                                  ("annot", fake), ("per_obj", fake), ("quality", fake), ("state", fake), ("stream", None))]
    for kw, text in ((dict(counts=None), "null pointer"), (dict(n_obj=None), "null pointer"), (dict(lengths=None), "null pointer"),
                     (dict(quality=None), "null pointer"), (dict(state=None), "go together"), (dict(annot=None), "go together"),
                     (dict(metric=3), "unknown metric 3"), (dict(metric=-1), "unknown metric -1"), (dict(n_seqs=0), "n_seqs 0"),
                     (dict(n_seqs=L.MAX_SEQS + 1), "n_seqs 129"), (dict(lengths=ints([4, 0])), "sequence 1"),
                     (dict(n_obj=ints([2, 0])), "video 1: n_obj 0"), (dict(n_obj=ints([33, 1])), "video 0: n_obj 33")):
        assert lib.ivosw_jf_reduce_ragged(*args(**kw)) == -1 and text in msg() and "ivosw_jf_reduce_ragged" in msg(), (kw, msg())
