"""ivosw_qa_augment on the MI355X against the numpy restatement of its sampling rule (tests/augment_ref.py): every comparison is bit for
bit.  Small shapes: widths that are and are not a multiple of 4, more than one workgroup per sample, upsampling, both frame kinds in one call, the edge taps of the RGBX8 source,
the selection launch, sample groups, the photometric clips, every refusal, the chain into AssessNet and the targets, graph capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ivos_w_amd import _lib as L
from ivos_w_amd import metrics
from ivos_w_amd.datasets import transforms_assess as T
from tests import augment_ref as R
from tests import qa_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ERR_ARG = -1
IDENT = R.IDENTITY


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def video(H, W, n=2, O=2, seed=0, u8=False):
    g = np.random.RandomState(seed)
    frames = g.randint(0, 256, (n, H, W, 4)).astype(np.uint8) if u8 else g.rand(n, 3, H, W).astype(F32)
    gt = g.randint(0, O + 1, (n, H, W)).astype(np.uint8)
    gt[:, H // 3:H // 3 + 2, W // 3:W // 3 + 3] = 1
    planes = g.randint(0, 256, (O, n, H, W)).astype(np.uint8)
    planes[:, :, ::2, ::3] = np.where(g.rand(O, n, (H + 1) // 2, (W + 2) // 3) < 0.5, 204, 205)       # the bytes on both sides of the threshold
    return dict(frames=frames, gt=gt, planes=planes, obj_ids=list(range(1, O + 1)))


def three_videos():
    return [video(7, 9, seed=1), video(16, 20, seed=2, u8=True), video(33, 65, seed=3)]


def on_device(videos, dev):
    out = []
    for v in videos:
        fr = torch.from_numpy(v["frames"]).to(dev)
        if v["frames"].dtype == np.uint8:
            from ivos_w_amd.models.assessment import PackedFrames
            fr = PackedFrames(fr)
        out.append((fr, torch.from_numpy(v["gt"]).to(dev), torch.from_numpy(v["planes"]).to(dev), v["obj_ids"]))
    return out


def random_maps(g, H, W, Ho, Wo):
    """Finite maps of every kind: the identity, the exact flip, integer translations, resizes, free affine maps, and maps that push most
    taps outside the source."""
    kx, ky = W / Wo, H / Ho
    return [IDENT, (-1., 0., W - 1., 0., 1., 0.), (1., 0., float(g.randint(-3, 4)), 0., 1., float(g.randint(-3, 4))),
            (kx, 0., 0.5 * kx - 0.5, 0., ky, 0.5 * ky - 0.5),
            (kx * g.uniform(.8, 1.2), g.uniform(-.3, .3), g.uniform(-3, 3), g.uniform(-.3, .3), ky * g.uniform(.8, 1.2), g.uniform(-3, 3)),
            (1., 0., W - 1.5, 0., 1., -(Ho - 1.25)), (3., 2., -40., 1., -5., 1000.), (0., 0., 2.5, 0., 0., 3.25)]


def mixed_samples(videos, Ho, Wo, seed):
    g = np.random.RandomState(seed)
    samples = []
    for v, vid in enumerate(videos):
        n, H, W = vid["gt"].shape
        maps = random_maps(g, H, W, Ho, Wo)
        for k, m in enumerate(maps):
            s = dict(v=v, f=k % n, o=k % 2, post=m, noise=float(g.uniform(-.05, .05)), contrast=float(g.uniform(.9, 1.1)))
            if k % 3 == 1:
                s["cands"] = [maps[(k + j) % len(maps)] for j in range(1 + k % 4)]
            samples.append(s)
    return samples


def device_call(dev, videos, samples, Ho, Wo):
    ds = T.DeviceSamples(on_device(videos, dev), [(s["v"], s["f"], s["o"]) for s in samples])
    out = T.augment(ds, samples, Ho, Wo)
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in out.items()}


def same(got, want, what=""):
    for k in ("chosen", "label", "mask", "prob", "img"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k].view(np.uint8 if got[k].dtype == np.uint8 else np.int32)
                                                                                 != want[k].view(np.uint8 if want[k].dtype == np.uint8 else np.int32))[:5])


# ---------------------------------------------------------------------------------------------- mixed batch
@pytest.mark.parametrize("Ho,Wo", [(8, 12), (5, 7), (48, 64)])
def test_mixed_video_batch_equals_the_restatement(dev, Ho, Wo):
    videos = three_videos()
    samples = mixed_samples(videos, Ho, Wo, seed=Ho)
    assert {videos[s["v"]]["frames"].dtype for s in samples} == {np.dtype(np.uint8), np.dtype(F32)} and len(samples) > 22   # three groups
    same(device_call(dev, videos, samples, Ho, Wo), R.augment(videos, samples, Ho, Wo), f"{Ho}x{Wo}")


# ---------------------------------------------------------------------------------------------- edge taps
@pytest.mark.parametrize("Wo", [20, 19])
def test_edge_taps_on_the_rgbx8_source(dev, Wo):
    """sx exactly -1, -0.5, 0, W - 1, W - 0.5 and W at x = 0 (and the same offsets in y): the taps x0 = -1 and x0 = W - 1 read one side as 0."""
    vid = video(16, 20, seed=5, u8=True)
    W, H = 20, 16
    samples = []
    for c in (-1., -.5, 0., W - 1., W - .5, float(W)):
        samples.append(dict(v=0, f=0, o=0, post=(1., 0., c, 0., 1., 0.)))
        samples.append(dict(v=0, f=1, o=1, post=(0., 0., c, 0., 1., 0.)))                       # every pixel of a row on that coordinate
    for c in (-1., -.5, 0., H - 1., H - .5, float(H)):
        samples.append(dict(v=0, f=1, o=0, post=(1., 0., 0., 0., 1., c)))
    samples.append(dict(v=0, f=0, o=0, post=(1., 0., 0., 0., 1., H - 1.)))
    samples.append(dict(v=0, f=0, o=0, post=(1., 0., -1., 0., 1., H - .5)))
    same(device_call(dev, [vid], samples, 16, Wo), R.augment([vid], samples, 16, Wo), f"edge {Wo}")


# ---------------------------------------------------------------------------------------------- selection
def test_selection_of_candidates(dev):
    H, W = 12, 16
    g = np.random.RandomState(9)
    base = video(H, W, n=3, O=1, seed=9)
    gt = np.zeros((3, H, W), np.uint8)
    gt[0, 4:7, 5:9] = 1                                                    # frame 0: one object in the middle
    gt[2] = 1                                                              # frame 1: the object absent; frame 2: nothing but the object
    base["gt"] = gt
    away, stay, shift = (1., 0., 100., 0., 1., 0.), (1., 0., 2., 0., 1., -1.), (1., 0., 0., 0., 1., 1.)
    flip = (-1., 0., W - 1., 0., 1., 0.)
    samples = [dict(v=0, f=0, o=0, cands=[away, away, stay, IDENT], post=flip, noise=.01, contrast=1.02),
               dict(v=0, f=0, o=0, cands=[away] * 12, post=flip, noise=.01, contrast=1.02),
               dict(v=0, f=1, o=0, cands=[stay, away], post=IDENT),       # all 0 either way: "no candidate" holds one value, so does `stay`
               dict(v=0, f=2, o=0, cands=[stay, IDENT, away], post=IDENT),  # all 1 untransformed: `stay` brings the border's 0 in, IDENT keeps one value
               dict(v=0, f=2, o=0, cands=[stay, shift], post=IDENT)]        # no candidate keeps one value: the fallback
    want = R.augment([base], samples, H, W)
    assert want["chosen"].tolist() == [2, 12, 0, 1, 2]
    got = device_call(dev, [base], samples, H, W)
    same(got, want, "selection")
    post_only = device_call(dev, [base], [dict(v=0, f=0, o=0, post=flip, noise=.01, contrast=1.02)], H, W)
    for k in ("img", "prob", "label", "mask"):
        assert got[k][1].tobytes() == post_only[k][0].tobytes(), k
    # n_cand = 0 everywhere: the selection launch is skipped, the workspace may be NULL (T.augment passes none)
    assert post_only["chosen"].tolist() == [0]
    del g


# ---------------------------------------------------------------------------------------------- groups
def test_sixty_five_samples_one_sample_and_thirty_two_videos(dev):
    videos = [video(6 + v % 3, 8 + v % 5, n=1, O=1, seed=20 + v, u8=bool(v % 2)) for v in range(32)]
    g = np.random.RandomState(1)
    samples = []
    for k in range(65):
        v = (k * 7) % 32
        s = dict(v=v, f=0, o=0, post=(1., float(g.uniform(-.1, .1)), float(g.randint(-2, 3)), 0., 1., float(g.uniform(-1, 1))),
                 noise=float(g.uniform(-.02, .02)), contrast=float(g.uniform(.97, 1.03)))
        if k % 5 == 0:
            s["cands"] = [(1., 0., 50., 0., 1., 0.), (1., 0., 1., 0., 1., 0.)]
        samples.append(s)
    assert lib().ivosw_qa_augment_ws_bytes(65) == 65 * 13 * 2 and lib().ivosw_qa_augment_ws_bytes(0) == 0
    same(device_call(dev, videos, samples, 8, 12), R.augment(videos, samples, 8, 12), "65 samples")
    same(device_call(dev, videos, samples[64:], 5, 7), R.augment(videos, samples[64:], 5, 7), "1 sample")


def lib():
    return L.lib()


# ---------------------------------------------------------------------------------------------- photometric
def test_noise_and_contrast_hit_both_clips(dev):
    vid = video(7, 9, seed=4)
    vid["frames"][0, :, 0, :4] = [0., 1., 0.5, 0.999]
    samples = [dict(v=0, f=0, o=0, post=IDENT, noise=n, contrast=c)
               for n, c in ((.5, 1.), (-.5, 1.), (0., 3.), (.25, 2.), (-.25, .5), (-2., 1.), (2., .25), (0., 0.), (.1, -1.))]
    want = R.augment([vid], samples, 7, 9)
    assert (want["img"][0] == 1).any() and (want["img"][1] == 0).any() and (want["img"][2] == 1).any() and (want["img"][6] == .25).all()
    same(device_call(dev, [vid], samples, 7, 9), want, "photometric")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_alone(dev):
    Ho, Wo, N = 8, 12, 2
    vids = on_device([video(7, 9, seed=1), video(16, 20, seed=2, u8=True)], dev)
    fill = dict(img=torch.full((N * 3 * Ho * Wo,), 7.5, device=dev), prob=torch.full((N * Ho * Wo,), 7.5, device=dev),
                label=torch.full((N * Ho * Wo,), 0xA5, dtype=torch.uint8, device=dev), mask=torch.full((N * Ho * Wo,), 0xA5, dtype=torch.uint8, device=dev),
                chosen=torch.full((N,), -7, dtype=torch.int32, device=dev), ws=torch.full((256,), 0xA5, dtype=torch.uint8, device=dev))
    msg = lambda: lib().ivosw_last_error().decode()                         # noqa: E731

    def call(vfn=None, sfn=None, **kw):
        ds = T.DeviceSamples(vids, [(0, 0, 0), (1, 1, 1)])
        table = (L.AugVideo * len(ds.videos))(*ds.videos)
        rows = (L.AugSample * N)()
        for k, (v, f, o) in enumerate(ds.samples):
            rows[k].v, rows[k].f, rows[k].o, rows[k].n_cand, rows[k].contrast = v, f, o, 1, 1.0
            for j in range(6):
                rows[k].post[j] = rows[k].cand[0][j] = IDENT[j]
        if vfn:
            vfn(table)
        if sfn:
            sfn(rows)
        a = dict(videos=table, n_videos=2, samples=rows, n=N, Ho=Ho, Wo=Wo, ws_bytes=256,
                 **{k: ctypes.c_void_p(t.data_ptr()) for k, t in fill.items()})
        a.update(kw)
        return lib().ivosw_qa_augment(a["videos"], a["n_videos"], a["samples"], a["n"], a["Ho"], a["Wo"], a["img"], a["prob"], a["label"],
                                      a["mask"], a["chosen"], a["ws"], a["ws_bytes"], L.stream_ptr(dev))

    def vset(i, **kw):
        return lambda t: [setattr(t[i], k, v) for k, v in kw.items()]

    def sset(i, **kw):
        return lambda r: [setattr(r[i], k, v) for k, v in kw.items()]

    def smap(i, which, j, val):
        def f(r):
            (r[i].post if which == "post" else r[i].cand[0])[j] = val
        return f
    frames1 = vids[1][0].rgbx.data_ptr()
    cases = [(dict(videos=None), "null videos"), (dict(samples=None), "null samples_host")] + \
        [({k: None}, f"null {k}") for k in ("img", "prob", "label", "mask", "chosen")] + \
        [(dict(n_videos=0), "n_videos 0"), (dict(n_videos=33), "n_videos 33"), (dict(n=0), "n_samples 0"), (dict(n=-1), "n_samples -1"),
         (dict(Ho=0), "Ho x Wo"), (dict(Wo=0), "Ho x Wo"), (dict(Ho=65536), "Ho x Wo"), (dict(Wo=65536), "Ho x Wo"),
         (dict(Ho=65535, Wo=65535), "Ho * Wo"), (dict(ws=None), "ws: workspace 0 <"), (dict(ws_bytes=51), "ws: workspace 51 < 52"),
         (dict(img=ctypes.c_void_p(vids[0][0].data_ptr())), "img overlaps the frames of video 0"),
         (dict(label=ctypes.c_void_p(vids[1][1].data_ptr() + 8)), "label overlaps the gt of video 1"),
         (dict(mask=ctypes.c_void_p(vids[1][2].data_ptr() + 100)), "mask overlaps the planes of video 1"),
         (dict(ws=ctypes.c_void_p(fill["prob"].data_ptr())), "prob overlaps ws"),
         (dict(ws=ctypes.c_void_p(vids[0][1].data_ptr() + 3)), "ws overlaps the gt of video 0"),
         (dict(ws=ctypes.c_void_p(vids[1][0].rgbx.data_ptr())), "ws overlaps the frames of video 1")]
    for kw, text in cases:
        assert call(**kw) == ERR_ARG and text in msg(), (kw, msg())
    for fn, text in ((vset(1, frames_kind=2), "video 1: unknown frames_kind 2"), (vset(1, frames=frames1 + 2), "video 1: frames off the 4-byte grid"),
                     (vset(0, frames=None), "video 0"), (vset(0, gt=None), "video 0"), (vset(1, planes=None), "video 1"),
                     (vset(0, n_obj=0), "video 0"), (vset(0, n_obj=33), "video 0"), (vset(1, H=0), "video 1"), (vset(1, n_frames=0), "video 1"),
                     (vset(0, H=1, W=(1 << 24) + 1), "video 0: null frames / gt / planes, n_frames, H or W < 1, H or W > 2^24")):
        assert call(vfn=fn) == ERR_ARG and text in msg(), msg()
    for fn, text in ((sset(1, v=2), "sample 1: video 2"), (sset(0, v=-1), "sample 0: video -1"), (sset(1, f=2), "sample 1: frame 2"),
                     (sset(0, f=-1), "sample 0: frame -1"), (sset(1, o=2), "sample 1: object 2"), (sset(0, o=-1), "sample 0: object -1"),
                     (sset(1, n_cand=13), "sample 1: n_cand 13"), (sset(0, n_cand=-1), "sample 0: n_cand -1"),
                     (sset(1, noise=float("nan")), "sample 1"), (sset(0, contrast=float("inf")), "sample 0"),
                     (smap(1, "post", 2, float("inf")), "sample 1"), (smap(0, "cand", 5, float("nan")), "sample 0")):
        assert call(sfn=fn) == ERR_ARG and text in msg() and ("sample" not in text or "samples_host" in msg()), msg()
    torch.cuda.synchronize(dev)
    for k, t in fill.items():
        assert bool((t == t[0]).all()) and t[0].item() in (7.5, 0xA5, -7), f"a refused call wrote {k}"
    assert call() == 0, msg()
    torch.cuda.synchronize(dev)
    assert not bool((fill["label"] == 0xA5).any()) and fill["chosen"].tolist() == [0, 0]
    assert bool((fill["ws"][:52] != 0xA5).sum() == 8) and bool((fill["ws"][52:] == 0xA5).all())      # 2 samples x 2 pairs x 2 flags


# ---------------------------------------------------------------------------------------------- chain
def test_chain_into_assessnet_and_the_targets(dev):
    import random
    from ivos_w_amd import synth
    from ivos_w_amd.models.assessment import AssessNet
    H, W = 32, 40
    vids_np = [video(H, W, n=3, O=2, seed=30), video(H, W, n=3, O=2, seed=31, u8=True)]
    for v in vids_np:                                                      # blobs, so that targets are not all degenerate
        v["gt"][:] = 0
        v["gt"][:, 8:20, 10:26] = 1
        v["gt"][:, 22:30, 4:14] = 2
        v["planes"][:] = np.where(v["gt"][None] == np.array([1, 2])[:, None, None, None], 230, 20) + (v["planes"] % 16)
    units = [(0, 0, 0), (0, 1, 1), (0, 2, 0), (1, 0, 1), (1, 1, 0), (1, 2, 1)]
    pipe = T.Compose([T.Resize(size=(W, H)), T.RandomAffine(), T.AdditiveNoise(), T.RandomContrast(), T.RandomHorizontalFlip(), T.ToTensor()])
    net = AssessNet(precision="fp32")
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0).items()})
    net.to(dev).eval()
    ds = T.DeviceSamples(on_device(vids_np, dev), units)
    random.seed(5)
    np.random.seed(5)
    rows, (Wo, Ho) = pipe.draw(ds.sizes())
    want = R.augment(vids_np, [dict(v=v, f=f, o=o, **r) for (v, f, o), r in zip(units, rows)], Ho, Wo)
    random.seed(5)
    np.random.seed(5)
    torch.cuda.synchronize(dev)
    # torch raises on every synchronising call IT makes in here (a .item(), a blocking copy, a synchronize in the Python wrapper); a
    # synchronisation inside the C call is invisible to it - that one is ruled out by the capture test below, where it would fail
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = pipe(ds)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    scores = net.forward(out["img"], out["prob"])
    res = metrics.qa_targets([(out["label"], out["mask"][None], 1)], "J_AND_F", scores=scores, thr=205)
    same({k: t.cpu().numpy() for k, t in out.items()}, want, "chain")
    # tests/qa_ref.py's loop on the restated batch with the same scores (the counts of the restated label / mask come from the project's own
    # count pass, which tests/test_gpu_qa.py holds to its references: what is checked independently here is the warp and the loop)
    counts, _, _ = metrics.qa_counts([(torch.from_numpy(want["label"]).to(dev), torch.from_numpy(want["mask"][None]).to(dev), 1)], 205)
    target, valid = qa_ref.unit_targets(counts.cpu().numpy().reshape(len(units), 1, 6), "J_AND_F")
    loss, diff, n_valid = qa_ref.report(scores.cpu().numpy(), target, valid)
    rep = res.report.cpu().numpy()
    assert n_valid == len(units) == int(rep[0, 2])
    assert F32(loss).tobytes() == rep[0, 0].tobytes() and F32(diff).tobytes() == rep[0, 1].tobytes()


# ---------------------------------------------------------------------------------------------- capture
def test_one_call_captured_and_replayed(dev):
    videos = three_videos()
    samples = mixed_samples(videos, 8, 12, seed=8)[:14]
    ds = T.DeviceSamples(on_device(videos, dev), [(s["v"], s["f"], s["o"]) for s in samples])
    want = T.augment(ds, samples, 8, 12)
    torch.cuda.synchronize(dev)
    want = {k: t.cpu().numpy() for k, t in want.items()}
    out = {k: torch.full(t.shape, 3, dtype=torch.from_numpy(t).dtype, device=dev) for k, t in want.items()}
    ws = T.workspace(len(samples), dev)                                    # the capture allocates nothing: outputs and workspace are the caller's
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        T.augment(ds, samples, 8, 12, out=out, ws=ws)
    for _ in range(2):
        for t in out.values():
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize(dev)
        same({k: t.cpu().numpy() for k, t in out.items()}, want, "replay")
