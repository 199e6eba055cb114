"""What the assessment-sample path costs on the device, against the only ways the parent had to the same bytes and numbers.

Conditions: 480p (480 x 854), 100 frames, 1 and 3 objects, all_P resident on the device in an object-major store.
  (a) bytes    device: metrics.quantize_probs + ONE uint8 copy to the host (misc.save_seg_preds without the file writing)
               host:   all_P.cpu() as float32, then (probs[:, 1:] * 255) and the saturating uint8 cast in numpy
  (b) report   device: quantise + counts from the planes + targets + the one copy of [loss, diff, n_valid] (utils_agent.assess_report)
               host:   all_P.cpu(), the bytes in numpy and their threshold (rint(p * 255) >= 205, what the reference's loop reads back from
                       its PNG files), then metrics.batched_jaccard / batched_f_measure once per object on binary maps and the reference
                       loop in numpy; the two ways are checked for equal [loss, diff, n_valid] while they are timed
  (c) kernel   ivosw_qa_quantize alone (device events), in TB/s over the 5 bytes per pixel it moves
  (d) counts   ivosw_qa_counts_videos from the planes against ivosw_jf_counts_videos on a label map of the same size (device events)
Host clock around chains that end in their synchronising copy; the ways alternate inside one process; medians of ROUNDS rounds with
min .. max.

    python tools/qa_probe.py [--out profiles/qa_probe.txt] [--rounds 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ivos_w_amd  # noqa: E402,F401
from ivos_w_amd import _lib as L  # noqa: E402
from ivos_w_amd import metrics  # noqa: E402
from ivos_w_amd.utils import utils_agent, utils_manet  # noqa: E402

H, W, N = 480, 854, 100
METRIC = "J_AND_F"


def make_session(dev, O, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    coarse = torch.randint(0, O + 1, (N, 12, 14), generator=g, dtype=torch.uint8).to(dev)
    gt = coarse.repeat_interleave(40, 1).repeat_interleave(61, 2)[:, :H, :W].contiguous()
    shifted = torch.roll(gt, (3, -5), (1, 2))
    store = utils_manet.ProbStore(N, O + 1, H, W, dev)
    logits = torch.randn(O + 1, N, H, W, device=dev)
    for c in range(O + 1):
        logits[c] += 4.0 * (shifted == c)
    store.buf.copy_(torch.softmax(logits, 0))
    pred = store.buf.argmax(0).to(torch.uint8).contiguous()
    scores = torch.rand(O, N, device=dev)
    return gt, pred, store, scores


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, r


def event_ms(fn, dev, reps=5):
    fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def fmt(xs):
    return f"{np.median(xs):9.3f}  ({min(xs):.3f} .. {max(xs):.3f})"


def host_bytes(store, O):
    p = store.all_P.cpu().numpy()
    with np.errstate(invalid="ignore"):
        return np.clip(np.rint(p[:, 1:] * np.float32(255)), 0, 255).astype(np.uint8)


def host_report(store, gt_host, scores_host, O):
    p = store.all_P.cpu().numpy()
    tot_l = tot_d = np.float32(0)
    cnt = 0
    for o in range(O):
        with np.errstate(invalid="ignore"):
            m = (np.clip(np.rint(p[:, o + 1] * np.float32(255)), 0, 255) >= 205).astype(np.uint8)
        g = (gt_host == o + 1).astype(np.uint8)
        j = metrics.batched_jaccard(g, m, average_over_objects=False, nb_objects=1)[:, 0]
        f = metrics.batched_f_measure(g, m, average_over_objects=False, nb_objects=1)[:, 0]
        t = (.5 * j + .5 * f).astype(np.float32)
        union = (g | m).reshape(N, -1).sum(1)
        for n in range(N):
            if union[n] > 0:
                e = np.float32(scores_host[o, n] - t[n])
                tot_l, tot_d, cnt = np.float32(tot_l + e * e), np.float32(tot_d + abs(e)), cnt + 1
    return np.asarray([tot_l / np.float32(max(cnt, 1)), tot_d / np.float32(max(cnt, 1)), cnt], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = L.lib()
    lines = [f"qa_probe: {H} x {W}, {N} frames, metric {METRIC}, medians of {args.rounds} alternating rounds (min .. max), ms",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    for O in (1, 3):
        gt, pred, store, scores = make_session(dev, O, 7 + O)
        gt_host, scores_host = gt.cpu().numpy(), scores.cpu().numpy()
        ta, tb = {"device": [], "host": []}, {"device": [], "host": []}
        dev_bytes = lambda: metrics.quantize_probs(store, O).cpu().numpy()
        dev_report = lambda: utils_agent.assess_report([(gt, store, O)], [scores], METRIC)[0][0]
        dev_bytes(), dev_report()                                        # warm-up (workspaces, pinned staging)
        for r in range(args.rounds):
            for way in (("device", "host") if r % 2 == 0 else ("host", "device")):
                ms, got = timed(dev_bytes if way == "device" else (lambda: host_bytes(store, O)), dev)
                ta[way].append(ms)
                if way == "device":
                    qb = got
                else:
                    assert np.array_equal(np.ascontiguousarray(got.transpose(1, 0, 2, 3)), qb), "device and host bytes differ"
            for way in (("device", "host") if r % 2 == 0 else ("host", "device")):
                ms, got = timed(dev_report if way == "device" else (lambda: host_report(store, gt_host, scores_host, O)), dev)
                tb[way].append(ms)
                if way == "device":
                    rep = got
                else:
                    assert np.array_equal(got, rep), f"host {got.tolist()} and device {rep.tolist()} reports differ"
                    same = f"equal, loss {rep[0]:.6f} diff {rep[1]:.6f} valid {int(rep[2])}"
        # (c) the kernel alone
        planes = torch.empty((O, N, H, W), dtype=torch.uint8, device=dev)
        q_ms = [event_ms(lambda: metrics._quantize_launch(store.all_P, O, planes), dev) for _ in range(args.rounds)]
        tbs = [5.0 * O * N * H * W / (ms * 1e-3) / 1e12 for ms in q_ms]
        # (d) the count pass: planes against the label map, alternating
        qv = L.QaVideo(gt=gt.data_ptr(), planes=planes.data_ptr(), n_frames=N, H=H, W=W, n_obj=O, bound_pix=int(metrics.bound_pixels((H, W))), thr=205)
        jv = L.JfVideo(gt=gt.data_ptr(), pred=pred.data_ptr(), n_frames=N, H=H, W=W, n_obj=O, bound_pix=int(metrics.bound_pixels((H, W))))
        for i in range(O):
            qv.obj_ids[i] = jv.obj_ids[i] = i + 1
        qt, jt = (L.QaVideo * 1)(qv), (L.JfVideo * 1)(jv)
        nbytes = lib.ivosw_jf_videos_ws_bytes(jt, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(N * O * 6, dtype=torch.int64, device=dev)
        st = L.stream_ptr(dev)
        from_planes = lambda: L.check(lib.ivosw_qa_counts_videos(qt, 1, L.dptr(counts), L.dptr(ws), nbytes, st), "qa_counts")
        from_labels = lambda: L.check(lib.ivosw_jf_counts_videos(jt, 1, L.dptr(counts), L.dptr(ws), nbytes, st), "jf_counts")
        tp, tl = [], []
        for r in range(args.rounds):
            for way in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tp if way == 0 else tl).append(event_ms(from_planes if way == 0 else from_labels, dev))
        lines += [f"--- {O} object(s): all_P {4 * (O + 1) * N * H * W / 1e6:.0f} MB float32, planes {O * N * H * W / 1e6:.0f} MB uint8",
                  f"(a) bytes to the host    device {fmt(ta['device'])}    host (float copy + numpy) {fmt(ta['host'])}"
                  f"    x{np.median(ta['host']) / np.median(ta['device']):.2f}",
                  f"(b) loss / diff report   device {fmt(tb['device'])}    host (copy, threshold, J / F per object) {fmt(tb['host'])}"
                  f"    x{np.median(tb['host']) / np.median(tb['device']):.2f}    results: {same}",
                  f"(c) ivosw_qa_quantize    {fmt(q_ms)} ms = {np.median(tbs):.2f} TB/s ({min(tbs):.2f} .. {max(tbs):.2f}) over 5 B / pixel"
                  f"  [float4 copy: 6.3 TB/s]",
                  f"(d) count pass           from planes {fmt(tp)}    from a label map (ivosw_jf_counts_videos) {fmt(tl)}"
                  f"    x{np.median(tp) / np.median(tl):.2f}", ""]
        del store, planes
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
