"""Entry-point runtime: what ``train_agent.py`` / ``eval_agent_{manet,atnet,ipn}.py`` at the repo root drive.

The reference's entry scripts (/root/reference/train_agent.py:119-379, eval_agent_manet.py:246-480) are sacred experiments
over the DAVIS-interactive session, a scribble robot and an external VOS clone.  None of those packages exists in this
image (sacred, easydict, davisinteractive, cv2, the MANet/ATNet/IPN clones, the DAVIS frames), so the scripts here are
written from scratch around the same loop

    session.next -> scribbles -> VOS segmentation -> sequence_metric -> recommend_frame -> submit_masks
                 -> [train: agent_business -> update_agent] -> summary.json / agent checkpoint

with two interchangeable back ends for the parts that are NOT on the hot path:

  * ``synthetic=1`` (default when the real stack is missing and ``synthetic`` was not set to 0): ``SyntheticDavis`` (seeded
    moving-blob videos with ground truth), ``SyntheticSession`` (the session protocol and the J&F curve bookkeeping of
    ``DavisInteractiveSession``; the "scribble" is the recommended frame's ground truth) and ``StandInVOS`` (a
    deterministic segmentation model whose error grows with the distance to the nearest annotated frame, producing
    stride-4 logits that go through the product's ``seg_epilogue`` kernel).
  * the real stack: refused with an explicit message listing what is missing (``require_real_stack``) — nothing is faked
    silently.

Everything ON the hot path is the product: AssessNet / Agent (HIP), ``recommend_frame``, ``agent_business``,
``sequence_metric`` (HIP J&F), ``ReplayMemory`` / ``load_agent_dataset``, ``save_agent_checkpoint``.
The CLI keeps sacred's ``with key=value`` form: ``python eval_agent_manet.py with setting=wild method=ours dataset=davis``.
"""
import contextlib
import copy
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch


class AttrDict(dict):
    """dict with attribute access (what the reference gets from easydict)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _attr(d):
    return AttrDict({k: _attr(v) if isinstance(v, dict) else v for k, v in d.items()})


# the keys the loop reads (the reference keeps them in configs/config.yaml); values are that file's defaults
DEFAULTS = dict(
    seed=0, gpu_id=0, phase="eval", setting="wild", method="ours", num_epochs=1, dataset="davis", ckpt_dir="weights",
    vos_adapter="",                    # module on PYTHONPATH that wraps the VOS backbone for the real stack (default ivosw_vos_<backbone>)
    synthetic=-1,                      # -1 auto (synthetic when the real stack is missing), 0 real stack only, 1 synthetic
    precision="bf16",                  # AssessNet mode: bf16 throughput (scores within 4e-3) / bf16x3 fast parity (1e-4) / fp32 exact parity
    frames="float32",                  # how the assessment path holds a video: "float32" [n,3,H,W] in 0..1 (the reference's all_F), or "uint8":
                                       # the decoded bytes packed as RGBX8 on the device (a quarter of the memory and of the upload; same scores
                                       # on the real stack, whose floats are bytes / 255)
    rescore="all",                     # the assessment pass of an interaction scores "all" (frame, object) units, or only the "changed" ones:
                                       # the device compares every mask plane with the session's copy of the planes it was last scored on and
                                       # the tower sees the units that differ (same scores; utils_agent.score_cache holds the copies)
    masks="float32",                   # how the assessment path holds a session's masks: "float32" probabilities [n,O+1,H,W] (the reference's
                                       # all_P), or "labels": ONE uint8 [n,H,W] map of hard labels (models.assessment.LabelMasks; 1 byte per pixel
                                       # and frame instead of 4 * (O + 1)) - the argmax of all_P, so its soft values are discarded
    metric="host",                     # where the oracle setting forms J / F and recommends: "host" (sequence_metric: the counts come back and
                                       # the ratios are formed in Python, then recommend_frame), or "device": ratios, per-frame means, the Brain's
                                       # state and the ranking in one device chain with one copy back (utils_agent.oracle_recommend; same values)
    overlay="none",                    # the pictures an annotator is shown, written after every interaction of the eval scripts: "none", or the
                                       # current masks drawn on the session's frames as "davis", "fade", "checker" or "color" (utils_ipn.overlay_session:
                                       # one device call and one copy back per interaction), under <report_dir>/overlays/
    overlay_frames="candidates",       # which frames are drawn then: the recommended "candidates", or "all" frames of the video
    save_probs=False,                  # true: after every interaction of the eval scripts the session's probability maps are written as 8-bit
                                       # planes under agent.save_result_dir, as the reference's generate_data.py writes AssessNet's training
                                       # samples (utils.misc.save_seg_preds: one quantise launch, one uint8 copy; refused under masks=labels)
    qa_report=False,                   # true (wild setting, method ours | worst): per interaction the reference's training-loop measures of the
                                       # AssessNet scores against the true per-unit targets - qa_loss (mean squared), qa_diff (mean absolute)
                                       # and valid/units - beside corr, and their session means under "qa" in summary.json
    qa_augment=False,                  # true (needs qa_report=true): the report line gains `aug loss .. diff .. n ..`, the same measures on ONE
                                       # augmented copy of every unit under the reference's train transform (Resize, RandomAffine, AdditiveNoise,
                                       # RandomContrast, RandomHorizontalFlip; datasets.transforms_assess: one fused warp on the device), seeded
                                       # from the run's seed, and "qa" in summary.json an "augmented" entry; false: no call, file or log line differs
    scribbles="frame",                 # what the synthetic session's robot hands out: "frame" (a scribble only names the annotated frame), or
                                       # "paths": one real polyline per object in davisinteractive's schema, drawn on the device at the stand-in's
                                       # logit resolution (utils.scribbles.scribble_maps) and fed to the stand-in VOS model
    robot="gt",                        # where the synthetic session's robot draws under scribbles=paths: "gt" (one straight run inside each object of
                                       # the ground truth, whatever was predicted), or "errors": along the skeleton of each object's error region
                                       # gt == o and pred != o of the masks last submitted, thinned on the device (utils.robot.interact)
    robot_min_nodes=4,                 # robot=errors: an error skeleton of fewer connected pixels draws no path (davisinteractive's min_nb_nodes)
    robot_background=False,            # robot=errors: true draws on the background too - paths of object 0 along the skeleton of the false
                                       # positives gt == 0 and pred != 0 (as davisinteractive's robot does), which tell the VOS model "this is
                                       # not an object"; false: no call, file or log line differs
    robot_paths="host",                # robot=errors: where the skeleton's pixels become paths: "host" (utils.robot.paths_from_points, numpy), or
                                       # "device": components, double BFS and resampling in one more launch (ivosw_robot_paths; the same paths)
                                       # and the stand-in's scribble map drawn straight from the device nodes; host: no call, file or log line differs
    report_save_dir="results",
    eval_max_nb_interactions=8,        # the eval scripts fix 8 interactions on the val subset (eval_agent_manet.py:64-65)
    data=dict(num_workers=0, root_dir_davis="data/DAVIS", root_dir_scribble_youtube_vos="data/Scribble_Youtube_VOS",
              subset="train", len_subseq=25),
    davis_interactive=dict(metric="J_AND_F", allow_repeat=1, max_nb_interactions=5, max_time_per_interaction=0, combine_th=0.4),
    agent=dict(save_result_dir="train", reward_csv="reward.csv", pretrain_csv="pretrain.csv", sample_th=0.05, optimizer="adam",
               lr=5e-6, lr_pow=0.9, momentum=0.9, weight_decay=5e-4, memory_size=100000, gamma=0.95, eps_start=0.7, eps_end=0.25,
               eps_k=5, eps_decay=500, update_rate=0.05, train_batch_size=32,
               loss="mse", huber_delta=1.0,    # DQN objective: the reference's two-term MSE, or "huber" (threshold huber_delta)
               nesterov=False,    # update: optimizer "adam" (the reference's) or "sgd" (clamp + SGD with momentum, nesterov)
               lr_schedule="constant", lr_total_steps=0,    # lr: constant (the reference's), or "poly": lr * (1 - min(k, N) / N) ** lr_pow
                                                            # at update k, N = lr_total_steps (required then)
               replay="uniform", per_alpha=0.6, per_beta=0.4, per_beta_steps=0, per_eps=1e-6,
                                   # minibatches: uniform (the reference's shuffle), or "prioritized": PER with priority exponent per_alpha,
                                   # IS exponent per_beta annealed to 1 over per_beta_steps draws (0: constant), per_eps added to |TD|
               target_update="coin", tau=0.005, target_period=20,
                                   # target net: "coin" (the reference's hard sync with probability update_rate per step), "soft" (Polyak
                                   # averaging with tau after every step) or "periodic" (hard sync every target_period-th step), on the device
               candidates=1, skip_annotated=False, candidate_gap=1),
                                   # recommendation: how many ranked frames the agent proposes per interaction (1: the reference's argmax; up
                                   # to 16), whether frames that were annotated before rank behind all others (select_next_frame's rule), and
                                   # the least distance in frames between any two of the candidates (1: the plain ranking)
    synth=dict(n_sequences=3, n_frames=30, height=120, width=216, max_objects=3, baseline_runs=30),
)


FRAME_MODES = ("float32", "uint8")


def frames_option(cfg):
    """cfg.frames (absent: "float32"), refused unless it is one of FRAME_MODES."""
    mode = cfg.get("frames", "float32")
    if not isinstance(mode, str) or mode not in FRAME_MODES:
        raise ValueError(f"frames must be 'float32' or 'uint8', got {mode!r}")
    return mode


MASK_MODES = ("float32", "labels")


def masks_option(cfg):
    """cfg.masks (absent: "float32"), refused unless it is one of MASK_MODES."""
    mode = cfg.get("masks", "float32")
    if not isinstance(mode, str) or mode not in MASK_MODES:
        raise ValueError(f"masks must be 'float32' or 'labels', got {mode!r}")
    return mode


OVERLAY_STYLES = ("none", "davis", "fade", "checker", "color")
OVERLAY_FRAMES = ("candidates", "all")


def overlay_option(cfg):
    """(cfg.overlay, cfg.overlay_frames) (absent: "none", "candidates"), refused unless they are one of OVERLAY_STYLES / OVERLAY_FRAMES."""
    style, which = cfg.get("overlay", "none"), cfg.get("overlay_frames", "candidates")
    if style is None:                                   # `overlay=none` on the command line reads as None (_coerce)
        style = "none"
    if not isinstance(style, str) or style not in OVERLAY_STYLES:
        raise ValueError(f"overlay must be 'none', 'davis', 'fade', 'checker' or 'color', got {style!r}")
    if not isinstance(which, str) or which not in OVERLAY_FRAMES:
        raise ValueError(f"overlay_frames must be 'candidates' or 'all', got {which!r}")
    return style, which


SCRIBBLE_MODES = ("frame", "paths")


def scribbles_option(cfg):
    """cfg.scribbles (absent: "frame"), refused unless it is one of SCRIBBLE_MODES."""
    mode = cfg.get("scribbles", "frame")
    if not isinstance(mode, str) or mode not in SCRIBBLE_MODES:
        raise ValueError(f"scribbles must be 'frame' or 'paths', got {mode!r}")
    return mode


ROBOT_MODES = ("gt", "errors")


def robot_option(cfg):
    """(cfg.robot, cfg.robot_min_nodes) (absent: "gt", 4).  Refused: a robot that is not one of ROBOT_MODES; robot=errors unless
    scribbles=paths (a scribble that only names its frame has nothing to draw); a robot_min_nodes that is not an integer >= 1."""
    mode, min_nodes = cfg.get("robot", "gt"), cfg.get("robot_min_nodes", 4)
    if not isinstance(mode, str) or mode not in ROBOT_MODES:
        raise ValueError(f"robot must be 'gt' or 'errors', got {mode!r}")
    if isinstance(min_nodes, bool) or not isinstance(min_nodes, int) or min_nodes < 1:
        raise ValueError(f"robot_min_nodes must be an integer >= 1, got {min_nodes!r}")
    if mode == "errors" and cfg.get("scribbles", "frame") != "paths":
        raise ValueError("robot=errors draws paths: it needs scribbles=paths")
    return mode, min_nodes


def robot_background_option(cfg):
    """cfg.robot_background (absent: False).  Refused: a value that is not a bool; true unless robot=errors (the ground-truth robot knows no
    prediction, so it has no false positive to draw on)."""
    on = cfg.get("robot_background", False)
    if not isinstance(on, bool):
        raise ValueError(f"robot_background must be true or false, got {on!r}")
    if on and cfg.get("robot", "gt") != "errors":
        raise ValueError("robot_background=true draws on the false positives of a prediction: it needs robot=errors")
    return on


ROBOT_PATHS_MODES = ("host", "device")


def robot_paths_option(cfg):
    """cfg.robot_paths (absent: "host").  Refused: a value that is not one of ROBOT_PATHS_MODES; "device" unless robot=errors (the
    ground-truth robot has no skeleton to walk)."""
    mode = cfg.get("robot_paths", "host")
    if not isinstance(mode, str) or mode not in ROBOT_PATHS_MODES:
        raise ValueError(f"robot_paths must be 'host' or 'device', got {mode!r}")
    if mode == "device" and cfg.get("robot", "gt") != "errors":
        raise ValueError("robot_paths=device walks the error skeletons on the device: it needs robot=errors")
    return mode


def qa_option(cfg):
    """(cfg.save_probs, cfg.qa_report) (absent: False, False).  Refused: a value that is not a bool; either key under phase=train (the
    training script has no such step); qa_report outside the wild setting
    with method ours | worst (no AssessNet scores exist elsewhere); save_probs under masks=labels (the soft values are gone)."""
    save_probs, qa_report = cfg.get("save_probs", False), cfg.get("qa_report", False)
    if not isinstance(save_probs, bool):
        raise ValueError(f"save_probs must be true or false, got {save_probs!r}")
    if not isinstance(qa_report, bool):
        raise ValueError(f"qa_report must be true or false, got {qa_report!r}")
    if (save_probs or qa_report) and cfg.get("phase", "eval") == "train":
        raise ValueError("save_probs / qa_report belong to the eval scripts (eval_agent_*.py, generate_data.py): train_agent.py would ignore them")
    if qa_report and not (cfg.get("setting") == "wild" and cfg.get("method") in ("ours", "worst")):
        raise ValueError(f"qa_report=true needs AssessNet's scores: setting=wild with method=ours or method=worst, got setting="
                         f"{cfg.get('setting')!r} method={cfg.get('method')!r}")
    if save_probs and cfg.get("masks", "float32") == "labels":
        raise ValueError("save_probs=true is refused under masks=labels: the soft probabilities are hardened to labels there, so there is "
                         "nothing to quantise (use masks=float32)")
    return save_probs, qa_report


def qa_augment_option(cfg):
    """cfg.qa_augment (absent: False).  Refused: a value that is not a bool; true without qa_report=true (the augmented measures extend
    the report, there is nothing to extend elsewhere)."""
    on = cfg.get("qa_augment", False)
    if not isinstance(on, bool):
        raise ValueError(f"qa_augment must be true or false, got {on!r}")
    if on and cfg.get("qa_report", False) is not True:
        raise ValueError("qa_augment=true needs qa_report=true: it adds the measures of the augmented samples to that report")
    return on


_QA_LABELS_NOTE = ("[ivos-w] qa_report under masks=labels: the soft values are gone, the report scores the one-hot planes of the label map "
                   "(255 where the label is the object, else 0)")


class QaSession:
    """What run_eval / run_eval_real do under save_probs / qa_report, one call per interaction (nothing is made when both are off).
    qa_report: the assessment passes' per-unit scores are tapped (utils_agent.score_tap), and ``after`` chains quantise -> counts from
    the planes -> targets on the device (utils_agent.assess_report) with one copy of [loss, diff, n_valid]."""

    def __init__(self, cfg, options, metric, masks):
        from .utils import misc, utils_agent
        self.save_probs, self.qa_report = options
        self.metric, self.masks, self.out_dir = metric, masks, cfg.agent.save_result_dir
        self.loss, self.diff, self.valid, self.units = misc.AverageMeter(), misc.AverageMeter(), 0, 0
        if self.qa_report:
            utils_agent.score_tap = []
            if masks == "labels":
                print(_QA_LABELS_NOTE)
        self.augment = None                                                # qa_augment: (assess_net, seed), set by enable_augment
        self.aug_frames = None                                             # the frames of the current sequence, set by the loop
        if self.save_probs:
            print(f"[ivos-w] save_probs=true: 8-bit probability planes of every interaction under {self.out_dir} (quantised on the device)")

    def enable_augment(self, assess_net, seed):
        """qa_augment=true: ``after`` also reports on one augmented copy of every unit (utils_agent.assess_report_augmented)."""
        from .utils import misc
        self.augment = (assess_net, int(seed))
        self.aug_loss, self.aug_diff, self.aug_valid, self.aug_calls = misc.AverageMeter(), misc.AverageMeter(), 0, 0
        print("[ivos-w] qa_augment=true: the report also scores one augmented copy of every unit (train transform, one fused warp on the device)")

    def _after_augmented(self, gt_masks, planes, n_objects):
        from .utils import utils_agent
        assess_net, seed = self.augment
        rep, _ = utils_agent.assess_report_augmented([(self.aug_frames, gt_masks, planes, n_objects)], assess_net, self.metric,
                                                     seed=seed + self.aug_calls)
        self.aug_calls += 1
        loss, diff, n_valid = float(rep[0, 0]), float(rep[0, 1]), int(rep[0, 2])
        if n_valid:
            self.aug_loss.update(loss)
            self.aug_diff.update(diff)
        self.aug_valid += n_valid
        return f"aug loss {loss:.4f} diff {diff:.4f} n {n_valid} "

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        """Releases the score tap whether the loop ended or raised: later assessment passes of the process keep nothing."""
        from .utils import utils_agent
        if self.qa_report:
            utils_agent.score_tap = None
        return False

    def after(self, sequence, visit, n_interaction, gt_masks, labels, all_P, n_objects, device):
        """-> the text that goes beside `corr` ("" without qa_report)."""
        from . import metrics
        from .utils import misc, utils_agent
        planes = None
        if self.masks != "labels":
            planes = metrics.quantize_probs(all_P, n_objects)              # one launch serves the files and the report
        if self.save_probs:
            misc.save_seg_preds(planes, dict(sequence=sequence, scribble_iter=visit, n_interaction=n_interaction), self.out_dir)
        if not self.qa_report:
            return ""
        scores, utils_agent.score_tap = utils_agent.score_tap, []
        if planes is None:                                                 # masks=labels: one-hot planes of the label map
            lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels), dtype=np.uint8))
            lab = lab.to(device=device, dtype=torch.uint8)
            ids = torch.arange(1, n_objects + 1, device=device, dtype=torch.uint8).view(-1, 1, 1, 1)
            planes = (lab.unsqueeze(0) == ids).to(torch.uint8) * 255
        rep, _ = utils_agent.assess_report([(gt_masks, planes, n_objects)], scores[-1:], self.metric)
        loss, diff, n_valid = float(rep[0, 0]), float(rep[0, 1]), int(rep[0, 2])
        units = int(planes.shape[0]) * int(planes.shape[1])
        if n_valid:
            self.loss.update(loss)
            self.diff.update(diff)
        self.valid += n_valid
        self.units += units
        text = f"qa_loss: {loss:.4f} qa_diff: {diff:.4f} valid: {n_valid}/{units} "
        if self.augment is not None:
            text += self._after_augmented(gt_masks, planes, n_objects)
        return text

    def summary(self):
        """The "qa" block of summary.json (None without qa_report)."""
        if not self.qa_report:
            return None
        out = {"loss": float(self.loss.avg), "diff": float(self.diff.avg), "valid": int(self.valid), "units": int(self.units)}
        if self.augment is not None:
            out["augmented"] = {"loss": float(self.aug_loss.avg), "diff": float(self.aug_diff.avg), "valid": int(self.aug_valid)}
        return out


def write_image(path_stem, rgb):
    """A uint8 [H,W,3] picture to ``path_stem`` + ".png" through PIL when it is importable, else + ".ppm" (binary P6) from plain Python.
    Returns the path written."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    try:
        from PIL import Image
    except ImportError:
        path = path_stem + ".ppm"
        with open(path, "wb") as fp:
            fp.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]) + rgb.tobytes())
        return path
    path = path_stem + ".png"
    Image.fromarray(rgb).save(path)
    return path


def write_overlays(overlay, report_dir, sequence, visit, interaction, all_F, labels, n_objects, candidates, device):
    """overlay = overlay_option(cfg).  Under a style other than "none": the candidate frames (or all frames) of the current session with
    the current masks drawn on them - ONE utils_ipn.overlay_session call and ONE device-to-host copy (labels handed in on the host, as
    the real stack's are, cost one upload first; the candidates are drawn once each, in ascending order) - written to
    <report_dir>/overlays/<sequence>_<visit>/<interaction>/<frame:05d>.png (.ppm without PIL).  Returns the paths written."""
    style, which = overlay
    if style == "none":
        return []
    from .utils import utils_agent, utils_ipn
    frames = utils_agent.frame_cache.get(all_F, device)               # the session's frames on the device (a PackedFrames is handed on)
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels), dtype=np.uint8))
    labels = labels.to(device=device, dtype=torch.uint8)
    ids = list(range(int(labels.shape[0]))) if which == "all" else sorted(set(int(f) for f in candidates))
    pics = utils_ipn.overlay_session(frames, labels, n_objects, style=style, frame_ids=ids).cpu().numpy()
    out_dir = os.path.join(report_dir, "overlays", f"{sequence}_{visit}", str(interaction))
    os.makedirs(out_dir, exist_ok=True)
    paths = [write_image(os.path.join(out_dir, f"{f:05d}"), pics[j]) for j, f in enumerate(ids)]
    print(f"[ivos-w] overlay={style}: {len(paths)} pictures of {sequence}_{visit}, interaction {interaction}, in {out_dir}")
    return paths


def _harden(all_P, masks):
    """What the recommender is handed in all_P's place: all_P itself, or under masks=labels its hard labels as a LabelMasks."""
    if masks != "labels":
        return all_P
    from .models.assessment import LabelMasks
    return LabelMasks.from_probs(all_P)


def rescore_option(cfg):
    """cfg.rescore (absent: "all"), refused unless it is "all" or "changed" (utils_agent.RESCORE_MODES)."""
    from .utils import utils_agent
    return utils_agent.rescore_option(cfg)


def metric_option(cfg):
    """cfg.metric (absent: "host"), refused unless it is "host" or "device" (utils_agent.METRIC_MODES)."""
    from .utils import utils_agent
    return utils_agent.metric_option(cfg)


def _print_metric_mode(cfg):
    mode = metric_option(cfg)
    print(f"[ivos-w] metric={mode}: " + ("J / F ratios, the per-frame means and the oracle recommendation run as one device chain "
                                         "(utils_agent.oracle_recommend), one copy back per interaction" if mode == "device" else
                                         "J / F counts on the device, ratios on the host (sequence_metric)"))


def _coerce(text):
    for cast in (int, float):
        try:
            return cast(text)
        except ValueError:
            pass
    return {"true": True, "false": False, "none": None}.get(text.lower(), text)


def parse_cli(argv, **overrides):
    """sacred's surface: ``script.py [--config file.yaml] [with] a=1 b.c=x``.  Unknown top-level keys are accepted (sacred adds
    them too); a dotted key must address an existing section."""
    cfg = copy.deepcopy(DEFAULTS)
    cfg.update(overrides)
    args = list(argv)
    if "--config" in args:
        import yaml
        i = args.index("--config")
        with open(args[i + 1]) as f:
            for k, v in (yaml.safe_load(f) or {}).items():
                if isinstance(v, dict) and isinstance(cfg.get(k), dict):
                    cfg[k].update(v)
                else:
                    cfg[k] = v
        del args[i:i + 2]
    for tok in args:
        if tok == "with":
            continue
        if "=" not in tok:
            raise SystemExit(f"unrecognised argument {tok!r}: expected `with key=value ...`")
        key, val = tok.split("=", 1)
        node, parts = cfg, key.split(".")
        for p in parts[:-1]:
            if not isinstance(node.get(p), dict):
                raise SystemExit(f"unknown config section {p!r} in {key!r}")
            node = node[p]
        node[parts[-1]] = _coerce(val)
    try:
        frames_option(cfg)
        masks_option(cfg)
        rescore_option(cfg)
        metric_option(cfg)
        cfg["overlay"] = overlay_option(cfg)[0]
        qa_option(cfg)
        qa_augment_option(cfg)
        scribbles_option(cfg)
        robot_option(cfg)
        robot_background_option(cfg)
        robot_paths_option(cfg)
    except ValueError as e:
        raise SystemExit(f"[ivos-w] {e}")
    return _attr(cfg)


# ------------------------------------------------------------------------------------------ the real stack, or a clear refusal
# What eval_agent_{manet,atnet,ipn}.py need besides this build: the davisinteractive package (session, scribble robot, Davis index),
# cv2 (frame decoding), the DAVIS frames, and the VOS backbone.  The backbone and its glue are third-party clones the reference
# keeps outside its own tree (README.md:35-41; SURVEY section 2 marks them OUT OF SCOPE): they enter through ONE small adapter module the
# caller puts on PYTHONPATH — ``cfg.vos_adapter`` (default ``ivosw_vos_<backbone>``) exposing
#
#     build(cfg, device) -> adapter
#     adapter.start_sequence(sequence, n_frame, n_objects, h, w)          once per (sequence, scribble) sample
#     adapter.segment(sequence, scribbles, annotated_frame, first_scribble, n_interaction)
#         -> (labels [n,H,W] integer label maps, all_P [n,O+1,H,W] float32 probabilities on the device)
#
# i.e. exactly what the reference's loop computes between "interaction initial" and "frame recommendation"
# (eval_agent_manet.py:321-396).  For MANet, ``ivos_w_amd.utils.utils_manet.get_results`` is the drop-in for the reference's
# get_results inside such an adapter.
REAL_STACK = ("davisinteractive", "cv2")


def adapter_module_name(backbone, cfg):
    return str(cfg.get("vos_adapter") or f"ivosw_vos_{backbone.lower()}")


def missing_real_stack(backbone, cfg):
    missing = []
    for mod in REAL_STACK + (adapter_module_name(backbone, cfg),):
        try:
            if mod not in sys.modules and importlib.util.find_spec(mod) is None:
                missing.append(f"python module {mod}")
        except (ImportError, ValueError):
            missing.append(f"python module {mod}")
    root = cfg.data.root_dir_davis
    if not os.path.isdir(os.path.join(root, "JPEGImages", "480p")):
        missing.append(f"DAVIS frames under {root}/JPEGImages/480p")
    return missing


def choose_backend(backbone, cfg):
    """-> True for the synthetic back end, False for the real stack (davisinteractive session + the caller's VOS adapter).
    ``synthetic=0`` with a missing stack stops with the list of what is missing."""
    missing = missing_real_stack(backbone, cfg)
    if cfg.synthetic == 1 or (cfg.synthetic == -1 and missing):
        if missing and cfg.synthetic == -1:
            print(f"[ivos-w] the {backbone} evaluation stack is not available here ({'; '.join(missing)}): running the SYNTHETIC "
                  "session with the stand-in VOS model (hot path = the product kernels). Pass synthetic=0 to insist on the real stack.")
        return True
    if missing:
        raise SystemExit(f"[ivos-w] synthetic=0 but the {backbone} stack is incomplete: " + "; ".join(missing))
    return False


# ------------------------------------------------------------------------------------------ synthetic data + session
class SyntheticDavis:
    """Seeded moving-blob videos with ground-truth label maps: the stand-in for davisinteractive.dataset.Davis + the frames."""

    def __init__(self, cfg, device):
        s, self.device = cfg.synth, device
        rs = np.random.RandomState(1000 + int(cfg.seed))
        self.dataset, self._params = {}, {}
        for i in range(int(s.n_sequences)):
            name = f"synth-{i:02d}"
            n_obj = 1 + rs.randint(int(s.max_objects))
            self.dataset[name] = dict(num_frames=int(s.n_frames), num_objects=n_obj, image_size=(int(s.width), int(s.height)))
            self._params[name] = dict(c0=rs.uniform(0.25, 0.75, (n_obj, 2)), v=rs.uniform(-0.012, 0.012, (n_obj, 2)),
                                      r=rs.uniform(0.10, 0.22, (n_obj, 2)), ph=rs.uniform(0, 6.28, n_obj),
                                      col=rs.uniform(0.2, 1.0, (n_obj + 1, 3)), seed=int(rs.randint(1 << 30)))
        self.sets = {cfg.data.subset: list(self.dataset)}
        self._cache = {}
        self.frames = frames_option(cfg)

    def _render(self, name):
        if name in self._cache:
            return self._cache[name]
        info, p = self.dataset[name], self._params[name]
        n, (w, h), O = info["num_frames"], info["image_size"], info["num_objects"]
        dev = self.device
        yy, xx = torch.meshgrid(torch.linspace(0, 1, h, device=dev), torch.linspace(0, 1, w, device=dev), indexing="ij")
        t = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
        label = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
        g = torch.Generator(device="cpu").manual_seed(p["seed"])
        frames = (0.35 + 0.1 * torch.rand(n, 3, h, w, generator=g)).to(dev)
        frames += 0.15 * torch.sin(12.0 * xx + 7.0 * yy)[None, None]
        for o in range(O):
            cy = float(p["c0"][o, 0]) + float(p["v"][o, 0]) * t + 0.05 * torch.sin(0.3 * t + float(p["ph"][o]))
            cx = float(p["c0"][o, 1]) + float(p["v"][o, 1]) * t + 0.05 * torch.cos(0.2 * t + float(p["ph"][o]))
            inside = ((yy[None] - cy) / float(p["r"][o, 0])) ** 2 + ((xx[None] - cx) / float(p["r"][o, 1])) ** 2 < 1.0
            label[inside] = o + 1
            col = torch.tensor(p["col"][o + 1], dtype=torch.float32, device=dev)[None, :, None, None]
            frames = torch.where(inside[:, None], 0.6 * col + 0.4 * frames, frames)
        self._cache[name] = (frames.clamp_(0, 1).cpu(), label)      # frames on the host, like the reference's all_F
        return self._cache[name]

    def load_frames(self, name):
        """float32 [n,3,H,W] on the host; under frames=uint8 the same frames quantised with round(f * 255), packed on the device."""
        frames = self._render(name)[0]
        if self.frames == "uint8":
            from .utils import utils_agent
            return utils_agent.pack_video((frames * 255.0).round().to(torch.uint8), self.device, layout="chw")
        return frames

    def load_annotations(self, name):
        return self._render(name)[1]                                  # uint8 [n,H,W] on the device (the J/F kernels read it there)


class SyntheticSession:
    """The protocol of DavisInteractiveSession as the entry scripts use it (next / get_scribbles / submit_masks /
    get_global_summary, ``samples``), with the J&F curve bookkeeping; a "scribble" names the annotated frame only, unless
    ``scribbles="paths"``: then the annotated frame's entry holds real paths - ``robot_paths`` on the ground truth, or with
    ``robot="errors"`` the paths of ``utils.robot.interact`` along the error skeletons of the masks last submitted for this sample
    (none yet: the objects themselves); ``robot_paths`` stands in only when no object at all yields a path.  ``drew`` names the robot
    that drew the last scribbles: "gt", "errors" or "gt (no error path)".  ``robot_background`` (with ``robot="errors"``): the error
    robot also draws paths of object 0 on the false positives of the masks last submitted (none before the first submission).
    ``robot_paths="device"`` (with ``robot="errors"``): the paths come from ``utils.robot.interact_device`` - the same list - and
    ``device_paths`` keeps the ``DevicePaths`` of the last scribbles (None when the error robot did not draw them)."""

    def __init__(self, davis, subset, metric_to_optimize, max_nb_interactions, report_save_dir, seed=0, rounds=1, scribbles="frame",
                 robot="gt", robot_min_nodes=4, robot_background=False, robot_paths="host"):
        self.robot_paths, self.device_paths = robot_paths, None
        self.davis, self.metric, self.max_nb = davis, metric_to_optimize, int(max_nb_interactions)
        self.scribble_mode = scribbles
        self.robot, self.robot_min_nodes, self.robot_background = robot, int(robot_min_nodes), bool(robot_background)
        self.drew, self._submitted = None, None
        self.report_save_dir = report_save_dir
        rs = np.random.RandomState(77 + seed)
        self.samples = [(seq, int(rs.randint(davis.dataset[seq]["num_frames"]))) for _ in range(rounds) for seq in davis.sets[subset]]
        self._i, self._k, self._frame = -1, 0, None
        self.records = []                                             # (sequence, sample index, interaction, mean metric, seconds)
        self._tic = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def next(self):
        if self._i >= 0 and 0 < self._k < self.max_nb:
            return True                                               # same sample, next interaction
        self._i += 1
        self._k = 0
        if self._i >= len(self.samples):
            return False
        self._frame = self.samples[self._i][1]
        self._submitted = None
        return True

    def get_scribbles(self, only_last=False):
        seq = self.samples[self._i][0]
        n = self.davis.dataset[seq]["num_frames"]
        mine = [dict(frame=self._frame)]
        if self.scribble_mode == "paths":
            gt, n_objects = self.davis.load_annotations(seq), self.davis.dataset[seq]["num_objects"]
            mine, self.drew = None, "gt"
            if self.robot == "errors":                                # every node of the skeleton path: the polyline stays on the error region
                from .utils import robot as R
                extra = dict(background=True) if self.robot_background else {}
                if self.robot_paths == "device":                      # interact(paths="device"), with the device nodes kept for the map
                    self.device_paths = R.interact_device(gt, self._submitted, n_objects, self._frame, min_nb_nodes=self.robot_min_nodes,
                                                          nb_points=None, **extra)
                    mine, self.drew = self.device_paths.to_scribbles(), "errors"
                else:
                    mine, self.drew = R.interact(gt, self._submitted, n_objects, self._frame, min_nb_nodes=self.robot_min_nodes,
                                                 nb_points=None, **extra), "errors"
                if not mine:
                    mine, self.drew, self.device_paths = None, "gt (no error path)", None
            if mine is None:
                mine = robot_paths(gt[self._frame].cpu().numpy(), n_objects)
        scribbles = dict(sequence=seq, annotated_frame=self._frame, scribbles=[mine if f == self._frame else [] for f in range(n)])
        self._tic = time.time()
        return seq, scribbles, self._k == 0

    def submit_masks(self, masks, next_scribble_frame_candidates=None):
        """masks: predicted labels [n,H,W] (device tensor or numpy).  The next scribble lands on the first candidate."""
        from .utils import misc
        seq = self.samples[self._i][0]
        gt = self.davis.load_annotations(seq)
        m = misc.sequence_metric(self.metric, gt, masks, self.davis.dataset[seq]["num_objects"])
        self._k += 1
        if self.robot == "errors":                                    # what the next scribble answers (a copy: the caller's store is rewritten)
            self._submitted = torch.as_tensor(masks, device=gt.device).to(torch.uint8).clone()
        self.records.append((seq, self._i, self._k, float(np.mean(m)), time.time() - (self._tic or time.time())))
        if next_scribble_frame_candidates:
            self._frame = int(next_scribble_frame_candidates[0])
        return m

    def get_global_summary(self):
        curve, times = [], []
        for k in range(1, self.max_nb + 1):
            vals = [r[3] for r in self.records if r[2] == k]
            curve.append(float(np.mean(vals)) if vals else float("nan"))
            times.append(float(np.mean([r[4] for r in self.records if r[2] == k])) if vals else 0.0)
        # like the package's curve, one trailing point beyond the last interaction (the scripts drop it with [:-1])
        return dict(curve={self.metric: curve + curve[-1:], "time": list(np.cumsum(times)) + [float(np.sum(times))]},
                    metric_at_threshold={self.metric: curve[-1], "threshold": 60})


def robot_paths(gt, n_objects, max_points=5):
    """The synthetic robot's scribbles on one ground-truth label map ``gt`` [H,W] (numpy), in davisinteractive's schema: one polyline
    ``dict(path=[[x, y], ...], object_id=o, start_time=0, end_time=0)`` per object o = 1 .. n_objects that has pixels on the frame, in
    ascending object order.  Construction, deterministic: the first of the object's rows that holds the most of its pixels; on that row
    the first of its longest runs of consecutive pixels, without a quarter of its length at either end (a robot draws inside the object,
    not along its edge); up to ``max_points`` pixels spread evenly from the first to the last pixel of what is left (``np.linspace``,
    rounded, duplicates dropped).  The polyline joins them in order, so every pixel it crosses is a pixel of the object.  A
    pixel (px, py) becomes the point ((px + 0.5) / W, (py + 0.5) / H), which maps back to it."""
    H, W = gt.shape
    paths = []
    for o in range(1, int(n_objects) + 1):
        mine = gt == o
        counts = mine.sum(1)
        if counts.max() == 0:
            continue
        y = int(counts.argmax())
        edges = np.flatnonzero(np.diff(np.concatenate(([0], mine[y].astype(np.int8), [0]))))      # run starts and ends, alternating
        starts, ends = edges[0::2], edges[1::2]
        k = int((ends - starts).argmax())
        inset = int(ends[k] - starts[k]) // 4
        x0, x1 = int(starts[k]) + inset, int(ends[k]) - 1 - inset
        xs = np.unique(np.linspace(x0, x1, min(int(max_points), x1 - x0 + 1)).round().astype(int))
        paths.append(dict(path=[[(float(x) + 0.5) / W, (y + 0.5) / H] for x in xs], object_id=o, start_time=0, end_time=0))
    return paths


class StandInVOS:
    """Deterministic stand-in for the VOS backbone: stride-4 logits whose error grows with the distance to the nearest annotated
    frame (the ground truth shifted by 1.5 px per frame of distance, plus seeded noise).  Annotated frames come out (almost) exact,
    so annotating the worst frame helps most — the structure the agent learns from.  ``scribble_low`` = (frame, int8 [h // 4, w // 4]
    scribble map on the device): the scribbled object's logit gains 8 at the scribbled low-resolution pixels of that frame (a scribble of
    object 0, which ``robot_background`` draws, raises channel 0: the background logit)."""

    def __init__(self, device, seed=0):
        self.device, self.seed = device, seed

    def logits(self, gt_u8, n_objects, annotated_frames, scribble_low=None):
        n, h, w = gt_u8.shape
        C = n_objects + 1
        onehot = torch.nn.functional.one_hot(gt_u8.long().clamp_(0, C - 1), C).permute(0, 3, 1, 2).float()
        low = torch.nn.functional.avg_pool2d(onehot, 4)
        ann = torch.as_tensor(sorted(set(int(a) for a in annotated_frames)), device=gt_u8.device)
        dist = (torch.arange(n, device=gt_u8.device)[:, None] - ann[None]).abs().min(1)[0]
        g = torch.Generator(device="cpu").manual_seed(self.seed + 31 * len(annotated_frames))
        noise = torch.randn(low.shape, generator=g).to(gt_u8.device)
        out = torch.empty_like(low)
        for f in range(n):
            d = int(dist[f])
            sh = int(round(1.5 * d / 4 * 4)) // 4 if d else 0
            out[f] = torch.roll(low[f], shifts=(sh, -sh), dims=(1, 2))
        res = 8.0 * (out - 0.5) + noise * (0.3 + 0.25 * dist.float())[:, None, None, None]
        if scribble_low is not None:                                  # device tensor work, no synchronisation
            frame, low_map = scribble_low
            lab = low_map.long()
            hit = ((lab >= 0) & (lab < C)).float()
            res[int(frame)] += 8.0 * hit[None] * torch.nn.functional.one_hot(lab.clamp(0, C - 1), C).permute(2, 0, 1).float()
        return res


# ------------------------------------------------------------------------------------------ building the hot-path objects
def build_hot_path(cfg, device, need_assess):
    from .models.agent import Agent
    from .models.assessment import AssessNet
    from .utils import misc
    agent = Agent(device=device, cfg=cfg)
    misc.load_agent_checkpoint(agent, cfg.ckpt_dir, device="cpu")      # never raises; random init when there is no file
    assess_net = None
    if need_assess:
        assess_net = AssessNet(precision=cfg.precision)
        ck = os.path.join(cfg.ckpt_dir, "assess_net.pt")
        if not misc.load_network_checkpoint(ck, assess_net, device="cpu"):
            from . import synth
            print(f"[ivos-w] no {ck}: AssessNet runs on the seeded synthetic weights")
            assess_net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()})
        assess_net = assess_net.to(device).eval()
    return agent, assess_net


def _segment(vos, davis, seq, n_objects, annotated, store, scribble_low=None):
    from .utils import utils_manet
    gt = davis.load_annotations(seq)
    lg = vos.logits(gt, n_objects, annotated, scribble_low=scribble_low)
    utils_manet.seg_epilogue(lg, gt.shape[1], gt.shape[2], store, 0)
    return store.labels_u8, store.all_P


def _print_rescored(rescore, needs_assess):
    """rescore=changed only: the share of (frame, object) units the assessment passes of the run scored again."""
    if rescore != "changed" or not needs_assess:
        return
    from .utils import utils_agent
    units, again = utils_agent.score_cache.stats()
    print(f"# rescore: changed  rescored {again} of {units} units ({100.0 * again / max(units, 1):.1f} %)")


_MASKS_NOTE = ("[ivos-w] masks=labels: the soft probabilities of every interaction are hardened to their argmax (one uint8 label map per "
               "session) before the assessment path sees them, so the numbers of this run differ from masks=float32")


# ------------------------------------------------------------------------------------------ eval_agent_*  (synthetic back end)
def run_eval(cfg, backbone="MANet"):
    """The loop of eval_agent_manet.py:246-480 on the synthetic back end.  Writes <report_save_dir>/summary.json =
    {"auc", "curve": {metric: [...]}} like the reference and returns it."""
    from .utils import misc, utils_agent, utils_manet
    frames = frames_option(cfg)                                        # (a bad value is refused here, before anything runs)
    masks = masks_option(cfg)
    rescore = rescore_option(cfg)
    overlay = overlay_option(cfg)
    qa = qa_option(cfg)
    qa_aug = qa_augment_option(cfg)
    scribble_mode = scribbles_option(cfg)
    robot, robot_min_nodes = robot_option(cfg)
    robot_background = robot_background_option(cfg)
    robot_paths = robot_paths_option(cfg)
    oracle_chain = metric_option(cfg) == "device" and cfg.setting == "oracle" and cfg.method in ("ours", "worst")
    cfg.phase = "eval"
    cfg.data.subset = "val"
    if not torch.cuda.is_available():
        raise SystemExit("[ivos-w] the hot path needs an MI355X (no CPU fallback)")
    device = torch.device(f"cuda:{cfg.gpu_id}")
    if not choose_backend(backbone, cfg):
        return run_eval_real(cfg, backbone, device)
    if frames == "uint8":
        print("[ivos-w] frames=uint8: the synthetic frames are quantised with round(f * 255) and packed as RGBX8 on the device, so the "
              "numbers of this run differ from frames=float32 (on the real stack the decoded frames ARE bytes and the two modes agree)")
    if masks == "labels":
        print(_MASKS_NOTE)
    misc.set_random_seed(int(cfg.seed))
    davis = SyntheticDavis(cfg, device)
    needs_assess = cfg.setting == "wild" and cfg.method in ("ours", "worst")
    agent, assess_net = build_hot_path(cfg, device, needs_assess)
    agent.set_eval()
    vos = StandInVOS(device, seed=int(cfg.seed))
    metric = cfg.davis_interactive.metric
    max_nb = int(cfg.eval_max_nb_interactions)
    report_dir = os.path.join(cfg.report_save_dir, backbone, cfg.setting, cfg.dataset, cfg.method)
    os.makedirs(report_dir, exist_ok=True)
    corr_all, rec_time, seen_seq = misc.AverageMeter(), misc.AverageMeter(), {}
    qa_sess = QaSession(cfg, qa, metric, masks) if any(qa) else None
    if qa_aug:
        qa_sess.enable_augment(assess_net, cfg.seed)
    with SyntheticSession(davis, cfg.data.subset, metric, max_nb, report_dir, seed=int(cfg.seed), scribbles=scribble_mode, robot=robot,
                          robot_min_nodes=robot_min_nodes, **(dict(robot_background=True) if robot_background else {}),
                          **(dict(robot_paths="device") if robot_paths == "device" else {})) as sess, \
            (qa_sess or contextlib.nullcontext()):
        while sess.next():
            sequence, scribbles, first_scribble = sess.get_scribbles(only_last=True)
            if first_scribble:
                info = davis.dataset[sequence]
                n_frame, n_objects = info["num_frames"], info["num_objects"]
                w, h = info["image_size"]
                next_frame = first_frame = scribbles["annotated_frame"]
                seen_seq[sequence] = seen_seq.get(sequence, 0) + 1
                all_F = davis.load_frames(sequence)                   # host tensor, built once per sequence (the frame cache key)
                prev_frames = None if cfg.davis_interactive.allow_repeat > 0 else [next_frame]
                annotated = [next_frame]
                quality_pred = np.zeros(n_frame) if needs_assess else None
                store = utils_manet.ProbStore(n_frame, n_objects + 1, h, w, device)
                n_interaction = 1
            else:
                annotated.append(next_frame)
                n_interaction += 1
            scribble_low, scribble_text = None, ""
            if scribble_mode == "paths":                              # the paths drawn at the stand-in's stride-4 logit resolution, as MANet
                from .utils import scribbles as S                     # draws them at its embedding resolution
                drawn = int(scribbles["annotated_frame"])
                if robot_paths == "device" and sess.device_paths is not None:     # the nodes never left the device: only the table goes up
                    from .utils import robot as R
                    scribble_low = (drawn, R.maps_from_paths(sess.device_paths, (h // 4, w // 4))[0])
                else:
                    scribble_low = (drawn, S.scribble_maps(scribbles, (h // 4, w // 4), frames=[drawn], device=device)[0])
                scribble_text = f"scribble: {len(scribbles['scribbles'][drawn])} paths "
                if robot == "errors":
                    scribble_text += f"robot: {sess.drew} "
                    if robot_paths == "device" and sess.device_paths is not None:
                        scribble_text += "(device paths) "
                    if robot_background:                              # (a path of object 0 raises the stand-in's background logit: channel 0)
                        n_bg = sum(1 for p in scribbles["scribbles"][drawn] if p.get("object_id") == 0)
                        scribble_text = scribble_text[:-1] + f" ({n_bg} background) "
            if scribble_low is None:                                  # (tests/test_qa_option.py replaces _segment by a six-argument double)
                labels, all_P = _segment(vos, davis, sequence, n_objects, annotated, store)
            else:
                labels, all_P = _segment(vos, davis, sequence, n_objects, annotated, store, scribble_low)
            if oracle_chain:                                          # metric=device: J / F, state, Brain and ranking in one device chain
                tic = time.time()
                qualities, picks = utils_agent.oracle_recommend(cfg, agent, device, [dict(
                    gt_masks=davis.load_annotations(sequence), pred_masks=labels, n_objects=n_objects,
                    annotated_frames_list=copy.deepcopy(annotated), prev_frames=prev_frames)], as_list=True)
                quality, candidates = qualities[0], [int(i) for i in picks[0]]
            else:
                quality = misc.sequence_metric(metric, davis.load_annotations(sequence), labels, n_objects)
                tic = time.time()
                candidates = [int(i) for i in utils_agent.recommend_candidates(cfg, assess_net, agent, device, [dict(
                    n_frame=n_frame, n_objects=n_objects, all_F=all_F, all_P=_harden(all_P, masks),
                    new_masks_quality=quality, prev_frames=prev_frames, annotated_frames_list=copy.deepcopy(annotated),
                    mask_quality=quality_pred, first_frame=first_frame, max_nb_interactions=max_nb)])[0]]
            next_frame = candidates[0]                                # the session annotates the first candidate
            if prev_frames is not None:
                prev_frames.append(next_frame)
            rec_time.update(time.time() - tic)
            if overlay[0] != "none":                                  # what the annotator is shown: the candidates with the current masks on them
                write_overlays(overlay, report_dir, sequence, seen_seq[sequence], n_interaction, all_F, labels, n_objects, candidates, device)
            sess.submit_masks(labels, next_scribble_frame_candidates=candidates)
            if qa_aug:
                qa_sess.aug_frames = all_F
            qa_text = "" if qa_sess is None else qa_sess.after(sequence, seen_seq[sequence], n_interaction, davis.load_annotations(sequence),
                                                               labels, all_P, n_objects, device)
            corr = float(np.corrcoef([quality, quality_pred])[0, 1]) if quality_pred is not None else float("nan")
            corr_all.update(0.0 if np.isnan(corr) else corr)
            print(f"avg_{metric}: {quality.mean() * 100:.2f} rec_time:{rec_time.val * 1e3:.1f} ms next_frame: {next_frame:2d} "
                  + (f"candidates: {candidates} " if len(candidates) > 1 else "") +
                  f"[{int((quality < quality[next_frame]).sum()) + 1:2d}/{n_frame:2d}] corr: {corr:.2f} {qa_text}{scribble_text}"
                  f"seq: {sequence}_{seen_seq[sequence]} [{n_interaction:2d}/{max_nb:2d}]")
        gs = sess.get_global_summary()
    curve = gs["curve"][metric][:-1]
    auc = float(np.trapz(curve) / (len(curve) - 1)) if len(curve) > 1 else float(curve[0])
    summary = {"auc": auc, "curve": {metric: curve}}
    if qa_sess is not None and qa_sess.qa_report:
        summary["qa"] = qa_sess.summary()
    with open(os.path.join(report_dir, "summary.json"), "w") as fp:
        json.dump(summary, fp)
    print(f"# global_summary: auc:{auc * 100:.4f}  recommend_frame avg {rec_time.avg * 1e3:.2f} ms  frame-cache uploads "
          f"{utils_agent.frame_cache.uploads}  frames: {frames}\n# {metric}: " + " ".join(f"{v * 100:.2f}" for v in curve))
    _print_rescored(rescore, needs_assess)
    summary["backend"] = "synthetic"
    summary["frames"] = frames
    summary["masks"] = masks
    summary["report_dir"] = report_dir
    return summary


# ------------------------------------------------------------------------------------------ eval_agent_*  (real stack)
def run_eval_real(cfg, backbone, device):
    """The loop of eval_agent_manet.py:246-480 on the REAL stack: davisinteractive's DavisInteractiveSession and scribble robot, the
    DAVIS frames from disk, the caller's VOS adapter for the segmentation, and this build's hot path for everything the reference
    owns in that loop: ``sequence_metric`` (J / F), ``recommend_frame`` (AssessNet + agent), the checkpoint loaders.  Writes
    <report_save_dir>/<backbone>/<setting>/<dataset>/<method>/summary.json like the reference (eval_agent_manet.py:470-480)."""
    if cfg.agent.get("candidates", 1) != 1:
        raise ValueError(f"agent.candidates = {cfg.agent.get('candidates')!r} is not supported on the real stack: its loop takes the "
                         "recommended frame for the annotated one, and davisinteractive's robot may pick any candidate (use 1)")
    import cv2
    from davisinteractive import utils as interactive_utils
    from davisinteractive.dataset import Davis
    from davisinteractive.session import DavisInteractiveSession
    from .utils import misc, utils_agent
    adapter_mod = importlib.import_module(adapter_module_name(backbone, cfg))
    frames = frames_option(cfg)
    masks = masks_option(cfg)
    rescore = rescore_option(cfg)
    metric_mode = metric_option(cfg)
    overlay = overlay_option(cfg)
    qa = qa_option(cfg)
    qa_aug = qa_augment_option(cfg)
    if masks == "labels":
        print(_MASKS_NOTE)
    misc.set_random_seed(int(cfg.seed))
    root = cfg.data.root_dir_davis
    needs_assess = cfg.setting == "wild" and cfg.method in ("ours", "worst")
    agent, assess_net = build_hot_path(cfg, device, needs_assess)
    agent.set_eval()
    vos = adapter_mod.build(cfg, device)
    metric = cfg.davis_interactive.metric
    max_nb = int(cfg.eval_max_nb_interactions)
    report_dir = os.path.join(cfg.report_save_dir, backbone, cfg.setting, cfg.dataset, cfg.method)
    os.makedirs(report_dir, exist_ok=True)
    davis = Davis(root)
    seen_seq, frames_of = {}, {}
    rec_time, corr_all, final_q = misc.AverageMeter(), misc.AverageMeter(), misc.AverageMeter()
    qa_sess = QaSession(cfg, qa, metric, masks) if any(qa) else None
    if qa_aug:
        qa_sess.enable_augment(assess_net, cfg.seed)
    with DavisInteractiveSession(host="localhost", davis_root=root, subset=cfg.data.subset, metric_to_optimize=metric,
                                 max_nb_interactions=max_nb, max_time=int(cfg.davis_interactive.max_time_per_interaction) or None,
                                 report_save_dir=report_dir) as sess, (qa_sess or contextlib.nullcontext()):
        while sess.next():
            sequence, scribbles, first_scribble = sess.get_scribbles(only_last=True)
            annotated = interactive_utils.scribbles.annotated_frames(scribbles)
            if first_scribble:
                n_objects = Davis.dataset[sequence]["num_objects"]
                gt_masks = davis.load_annotations(sequence)
                assert len(annotated) > 0
                next_frame = first_frame = annotated[0]
                seen_seq[sequence] = seen_seq.get(sequence, 0) + 1
                if sequence not in frames_of:                  # decoded once per sequence: also the key of the device frame cache
                    frames_of.clear()                          # davisinteractive serves a sequence's samples consecutively: keep ONE decoded
                                                               # video (0.35 GB of fp32 at 480p), as the reference holds one all_F — not the whole set
                                                               # (frames=uint8: 0.16 GB of RGBX8 bytes on the device and no host copy)
                    jdir = os.path.join(root, "JPEGImages", "480p", sequence)
                    if frames == "uint8":                      # cv2's bytes, BGR -> RGB, packed on the device: the same values as below
                        frames_of[sequence] = utils_agent.pack_video(
                            np.stack([np.asarray(cv2.imread(os.path.join(jdir, f)), dtype=np.uint8)[:, :, [2, 1, 0]] for f in sorted(os.listdir(jdir))],
                                     0), device)
                    else:
                        frames_of[sequence] = torch.from_numpy(np.ascontiguousarray(np.stack(
                            [np.asarray(cv2.imread(os.path.join(jdir, f)), dtype=np.float32)[:, :, [2, 1, 0]] / 255. for f in sorted(os.listdir(jdir))],
                            0).transpose(0, 3, 1, 2)))
                all_F = frames_of[sequence]
                n_frame = len(scribbles["scribbles"])
                h, w = (all_F.H, all_F.W) if frames == "uint8" else (int(all_F.shape[2]), int(all_F.shape[3]))
                prev_frames = None if cfg.davis_interactive.allow_repeat > 0 else [next_frame]
                annotated_list = [next_frame]
                quality_pred = np.zeros(n_frame) if needs_assess else None
                vos.start_sequence(sequence, n_frame, n_objects, h, w)
                n_interaction = 1
            else:
                annotated_list.append(next_frame)
                n_interaction += 1
            scribbles["annotated_frame"] = next_frame
            with torch.no_grad():
                labels, all_P = vos.segment(sequence, scribbles, next_frame, first_scribble, n_interaction)
            new_masks = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
            if metric_mode == "device":                               # the ratios and the means on the device, one copy back
                quality = misc.sequence_metric_videos(metric, [(gt_masks, labels if torch.is_tensor(labels) else new_masks, n_objects)])[0]
            else:
                quality = misc.sequence_metric(metric, gt_masks, new_masks, n_objects)
            tic = time.time()
            next_frame = int(utils_agent.recommend_frame(
                cfg, assess_net, agent, device, n_frame=n_frame, n_objects=n_objects, all_F=all_F, all_P=_harden(all_P, masks),
                new_masks_quality=quality,
                prev_frames=prev_frames, annotated_frames_list=copy.deepcopy(annotated_list), mask_quality=quality_pred,
                first_frame=first_frame, max_nb_interactions=max_nb))
            if prev_frames is not None:
                prev_frames.append(next_frame)
            rec_time.update(time.time() - tic)
            if overlay[0] != "none":
                write_overlays(overlay, report_dir, sequence, seen_seq[sequence], n_interaction, all_F, labels, n_objects, [next_frame], device)
            sess.submit_masks(new_masks, next_scribble_frame_candidates=[next_frame])
            if qa_aug:
                qa_sess.aug_frames = all_F
            qa_text = "" if qa_sess is None else qa_sess.after(sequence, seen_seq[sequence], n_interaction, gt_masks, labels, all_P, n_objects,
                                                               device)
            corr = float(np.corrcoef([quality, quality_pred])[0, 1]) if quality_pred is not None else float("nan")
            corr_all.update(0.0 if np.isnan(corr) else corr)
            print(f"avg_{metric}: {quality.mean() * 100:.2f} rec_time:{rec_time.val:.2f} next_frame: {next_frame:2d} "
                  f"[{int((quality < quality[next_frame]).sum()) + 1:2d}/{n_frame:2d}] corr: {corr:.2f} ({corr_all.avg:.2f}) {qa_text}"
                  f"seq: {sequence}_{seen_seq[sequence]} [{n_interaction:2d}/{max_nb:2d}]")
            if n_interaction == max_nb:
                final_q.update(float(quality.mean()) * 100)
        gs = sess.get_global_summary()
    curve = list(gs["curve"][metric][:-1])
    auc = float(np.trapz(curve) / (len(curve) - 1)) if len(curve) > 1 else float(curve[0])
    summary = {"auc": auc, "curve": {metric: curve}}
    if qa_sess is not None and qa_sess.qa_report:
        summary["qa"] = qa_sess.summary()
    with open(os.path.join(report_dir, "summary.json"), "w") as fp:
        json.dump(summary, fp)
    print(f"# final avg {metric}: {final_q.avg:.4f}  final avg corr: {corr_all.avg:.4f}\n# global_summary: auc:{auc * 100:.4f}  frames: {frames}\n"
          f"# {metric}: " + " ".join(f"{v * 100:.2f}" for v in curve))
    _print_rescored(rescore, needs_assess)
    summary["backend"] = "real"
    summary["frames"] = frames
    summary["masks"] = masks
    summary["report_dir"] = report_dir
    return summary


# ------------------------------------------------------------------------------------------ train_agent (synthetic back end)
def _episode(cfg, davis, vos, sess, agent, device, df, train_loader_fn, policy, seen=None):
    """Interactions of ONE session sample on a len_subseq window, reference flow (train_agent.py:150-330): oracle state
    (true J&F), recommend -> submit -> agent_business.  ``policy`` = 'random' (baseline / pretrain collection) or 'ours'."""
    from .utils import misc, utils_agent, utils_manet
    metric, max_nb = cfg.davis_interactive.metric, int(cfg.davis_interactive.max_nb_interactions)
    out = dict(losses=[], rewards_done=[], finals=[])
    state = dict(seen=seen if seen is not None else {})
    while sess.next():
        sequence, scribbles, first_scribble = sess.get_scribbles(only_last=False)
        if first_scribble:
            info = davis.dataset[sequence]
            n_objects = info["num_objects"]
            w, h = info["image_size"]
            state["seen"][sequence] = state["seen"].get(sequence, 0) + 1
            first_frame = scribbles["annotated_frame"]
            len_subseq = min(int(cfg.data.len_subseq), info["num_frames"])
            subseq = utils_agent.gen_subseq(first_frame, info["num_frames"], len_subseq)
            gt = davis.load_annotations(sequence)[torch.as_tensor(subseq, device=device)].contiguous()
            next_frame = subseq.index(first_frame)
            prev_frames, annotated = [next_frame], [next_frame]
            store = utils_manet.ProbStore(len_subseq, n_objects + 1, h, w, device)
            n_interaction, old_frame, old_meta, old_metric, repeat = 1, None, None, None, None
            loader = train_loader_fn(state["seen"][sequence]) if train_loader_fn else None
        else:
            counts = np.zeros(len(new_metric))
            for i in annotated:
                counts[i] += 1
            repeat = next_frame not in list(np.where(counts == counts.min())[0])
            annotated.append(next_frame)
            old_frame, old_meta, old_metric = next_frame, new_meta, new_metric
            n_interaction += 1
        lg = vos.logits(gt, n_objects, annotated)
        utils_manet.seg_epilogue(lg, h, w, store, 0)
        rcfg = AttrDict(cfg, setting="oracle" if policy == "ours" else "wild", method=policy)
        if policy == "ours" and metric_option(cfg) == "device":      # metric=device: J / F, state, Brain and argmax in one device chain
            metrics_, picks = utils_agent.oracle_recommend(rcfg, agent, device, [dict(
                gt_masks=gt, pred_masks=store.labels_u8, n_objects=n_objects, annotated_frames_list=copy.deepcopy(annotated),
                prev_frames=prev_frames)])
            new_metric, next_frame = metrics_[0], int(picks[0])
        else:
            new_metric = misc.sequence_metric(metric, gt, store.labels_u8, n_objects)
            next_frame = int(utils_agent.recommend_frame(
                rcfg, None, agent, device, n_frame=len_subseq, n_objects=n_objects, all_F=None, all_P=store.all_P,
                new_masks_quality=new_metric, prev_frames=prev_frames, annotated_frames_list=copy.deepcopy(annotated), mask_quality=None,
                first_frame=next_frame, max_nb_interactions=max_nb))
        prev_frames.append(next_frame)
        full = davis.load_annotations(sequence).clone()
        full[torch.as_tensor(subseq, device=device)] = store.labels_u8
        sess.submit_masks(full, next_scribble_frame_candidates=[subseq[next_frame]])
        new_meta = dict(sequence=sequence, scribble_iter=state["seen"][sequence], n_interaction=n_interaction)
        loss, r_step, r_done = utils_agent.agent_business(
            cfg, agent, max_nb, n_interaction, first_scribble=first_scribble, old_masks_metric=old_metric, new_masks_metric=new_metric,
            old_frame=old_frame, next_frame=next_frame, sequence=sequence, seen_seq=state["seen"], repeat_selection=repeat, df=df,
            annotated_frames_list=annotated, old_masks_meta=old_meta, new_masks_meta=new_meta,
            report_save_dir=cfg.agent.save_result_dir, agent_train_loader=loader)
        if n_interaction == max_nb:
            out["finals"].append(float(new_metric.mean()))
            out["rewards_done"].append(float(r_done))
            if float(loss) > 0:
                out["losses"].append(float(loss))
    return out


def bootstrap_synthetic_pool(cfg, davis, vos, device):
    """What the reference's baseline + pretrain phases leave on disk before train_agent.py starts (train_agent.py:90-97):
    ``reward.csv`` (30 random-policy episodes per (sequence, scribble_iter % 3): the reward baseline) and ``pretrain.csv``
    (their transitions: the initial replay pool) — produced here by running the random policy on the synthetic session."""
    import pandas as pd
    from .models.agent import Agent
    save_dir = cfg.agent.save_result_dir
    os.makedirs(save_dir, exist_ok=True)
    scratch = AttrDict(cfg, phase="pretrain")
    collector = Agent(device=device, cfg=scratch)
    collector.memory_pool.csv_sync_every = 256
    runs = int(cfg.synth.baseline_runs)
    sess = SyntheticSession(davis, cfg.data.subset, cfg.davis_interactive.metric, cfg.davis_interactive.max_nb_interactions, save_dir,
                            seed=1234, rounds=3 * runs)
    _episode(scratch, davis, vos, sess, collector, device, None, None, "random")
    collector.memory_pool.sync_csv(save_dir)
    pool = os.path.join(save_dir, collector.memory_pool.basename_csv)
    df = pd.read_csv(pool, index_col=0)
    df.to_csv(os.path.join(save_dir, cfg.agent.reward_csv))
    df.to_csv(os.path.join(save_dir, cfg.agent.pretrain_csv))
    return len(df)


def run_train(cfg):
    """train_agent.py:119-379 on the synthetic back end: replay pool from pretrain.csv, epochs over the session in the
    oracle/ours setting, agent_business -> update_agent at the end of every episode, agent.pt per epoch."""
    import pandas as pd
    from torch.utils.data import DataLoader
    from .datasets.agent_dataset import load_agent_dataset
    from .models.agent import Agent
    from .utils import misc
    cfg.phase = "train"
    if not torch.cuda.is_available():
        raise SystemExit("[ivos-w] the hot path needs an MI355X (no CPU fallback)")
    # Data parallel (BASELINE configs[3]; the reference has none, models/agent.py:90-92 is commented out): launched under
    # torch.distributed.run, every rank plays the SAME episodes (same seeds -> the same experience, the same replay pool, the same
    # epsilon / target-sync coins) and the exchange happens in the update loop: the shuffled minibatches of an episode are dealt
    # out to the ranks (parallel.RankBatchSampler), gradients are summed over the ranks and averaged inside clamp + Adam
    # (Agent.apply_gradients).  Rank 0 alone writes agent.pt / memory_pool.csv / the summaries into the configured directories;
    # the other ranks keep their (identical) working files under <save_result_dir>/rank<r>.
    from . import parallel
    prioritized = Agent._replay_option(cfg.agent)[0] == "prioritized"         # (a bad PER option is refused here, before anything runs)
    Agent._target_option(cfg.agent)                                           # (so is a bad target option; every mode runs data-parallel)
    if prioritized and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or parallel.forced()):
        raise SystemExit("[ivos-w] agent.replay=prioritized runs on one GPU only: every rank's TD errors would update its own sum tree "
                         "and the replicas would diverge (data-parallel PER needs an all-gather of the drawn rows and TD errors)")
    rank, world = 0, 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        rank, world, device = parallel.init()
        if rank > 0:
            sys.stdout = open(os.devnull, "w")
    else:
        device = torch.device(f"cuda:{cfg.gpu_id}")
    if not choose_backend("ATNet", cfg):                               # the reference trains against ATNet
        raise SystemExit("[ivos-w] train_agent.py drives the synthetic session only: training against the real ATNet clone needs the "
                         "reference's run_VOS_singleiact glue (utils/utils_atnet.py, out of scope - SURVEY section 2); evaluate a trained "
                         "agent on the real stack with eval_agent_*.py synthetic=0, or run with synthetic=1.")
    cfg.data.subset = cfg.data.get("subset", "train")
    misc.set_random_seed(2019)
    davis = SyntheticDavis(cfg, device)
    vos = StandInVOS(device, seed=int(cfg.seed))
    shared_dir = cfg.agent.save_result_dir
    p_reward, p_pre = os.path.join(shared_dir, cfg.agent.reward_csv), os.path.join(shared_dir, cfg.agent.pretrain_csv)
    if rank == 0 and not (os.path.exists(p_reward) and os.path.exists(p_pre)):
        n = bootstrap_synthetic_pool(cfg, davis, vos, device)
        print(f"[ivos-w] bootstrapped {p_reward} / {p_pre} from random-policy episodes ({n} transitions)")
    if world > 1:
        torch.distributed.barrier()
        if rank > 0:
            import shutil
            cfg.agent.save_result_dir = os.path.join(shared_dir, f"rank{rank}")
            os.makedirs(cfg.agent.save_result_dir, exist_ok=True)
            for src in (p_reward, p_pre):
                shutil.copy(src, cfg.agent.save_result_dir)
            p_reward, p_pre = (os.path.join(cfg.agent.save_result_dir, os.path.basename(q)) for q in (p_reward, p_pre))
    save_dir = cfg.agent.save_result_dir
    misc.set_random_seed(2019)                                         # the bootstrap consumed rank 0's streams: re-align every rank
    agent = Agent(device=device, cfg=cfg)
    df = pd.read_csv(p_reward, index_col=0)
    agent.memory_pool.load_from_csv(p_pre, save_dir, cfg.agent.sample_th)
    print(f"init memory pool from {p_pre}, now the size of memory pool is: {len(agent.memory_pool)}")
    davis.sets[cfg.data.subset] = [s for s in agent.memory_pool.seq_list if s in davis.dataset] or list(davis.dataset)
    misc.set_random_seed(2019)
    cache = {}

    def loader_for(seen):
        if (seen - 1) % 3 == 0 or "ds" not in cache:
            cache["ds"] = load_agent_dataset(cfg, agent.memory_pool.seq_list)
        if world > 1:
            seed = int(torch.empty((), dtype=torch.int64).random_().item() & 0x7fffffff)      # the global stream is the same on every rank
            return DataLoader(cache["ds"], num_workers=0,
                              batch_sampler=parallel.RankBatchSampler(len(cache["ds"]), int(cfg.agent.train_batch_size), rank, world, seed))
        return DataLoader(cache["ds"], batch_size=int(cfg.agent.train_batch_size), shuffle=True, num_workers=0)
    history, seen_seq = [], {}
    for epoch in range(1, int(cfg.num_epochs) + 1):
        agent.set_train()
        sess = SyntheticSession(davis, cfg.data.subset, cfg.davis_interactive.metric, cfg.davis_interactive.max_nb_interactions,
                                save_dir, seed=epoch, rounds=3)
        out = _episode(cfg, davis, vos, sess, agent, device, df, loader_for, "ours", seen_seq)
        if rank == 0:
            misc.save_agent_checkpoint(agent.policy_net, ckpt_dir=cfg.ckpt_dir)
        gs = sess.get_global_summary()
        curve = gs["curve"][cfg.davis_interactive.metric][:-1]
        auc = float(np.trapz(curve) / (len(curve) - 1))
        history.append(dict(epoch=epoch, auc=auc, final=float(np.mean(out["finals"])), agent_loss=float(np.mean(out["losses"])) if out["losses"] else 0.0,
                            reward_done=float(np.mean(out["rewards_done"])), updates=agent.optimizer.state["step"],
                            lr=agent.optimizer.current_lr()))       # the lr of the next update (the schedule's, at `updates`)
        per_note = ""
        if prioritized and agent.per_replay is not None:                # beta of the next draw, and the largest priority seen so far
            history[-1].update(per_beta=agent.per_replay.beta_next(), per_max_priority=agent.per_replay.max_priority())
            per_note = f" per_beta: {history[-1]['per_beta']:.6g} per_max_priority: {history[-1]['per_max_priority']:.6g}"
        history[-1].update(target_update=agent.target_update)
        tgt_note = f" target: {agent.target_update}"
        if agent.target_update == "periodic":                           # hard syncs so far: one every target_period-th update
            history[-1].update(target_syncs=agent.target_steps // agent.target_period)
            tgt_note += f" syncs: {history[-1]['target_syncs']}"
        print(f"# epoch {epoch}: auc:{auc:.4f} final {cfg.davis_interactive.metric}: {history[-1]['final'] * 100:.2f} agent loss: "
              f"{history[-1]['agent_loss']:.4f} reward_done: {history[-1]['reward_done']:.3f} updates: {history[-1]['updates']} "
              f"lr: {history[-1]['lr']:.6g}{per_note}{tgt_note}")
    if world > 1:
        # replicas must be bit-identical: compare an exact integer checksum of the parameter bits on every rank
        bits = agent.policy_net.flat.detach().view(torch.int32).to(torch.int64)
        chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 1009 + 1)).sum()])
        if torch.distributed.get_backend() == "gloo":
            chk = chk.cpu()
        got = [torch.empty_like(chk) for _ in range(world)]
        torch.distributed.all_gather(got, chk)
        same = all(bool(torch.equal(g, got[0])) for g in got)
        for h in history:
            h.update(world=world, replicas_identical=same, collective=parallel.collective_path(agent.policy_net.flat_grad))
        for v in list(parallel._P2P.values()):
            if v is not None:
                v.close()
        parallel._P2P.clear()
        if not same:
            raise SystemExit(f"[ivos-w] rank {rank}: the data-parallel replicas diverged (parameter checksums differ)")
    if rank == 0:
        with open(os.path.join(save_dir, "train_summary.json"), "w") as fp:
            json.dump(history, fp)
    return history


def main_eval(backbone, argv=None):
    cfg = parse_cli(sys.argv[1:] if argv is None else argv)
    _print_metric_mode(cfg)
    return run_eval(cfg, backbone)


def main_generate(argv=None):
    """generate_data.py: the eval loop on the synthetic back end with save_probs=true - AssessNet's training samples as 8-bit planes."""
    cfg = parse_cli(["synthetic=1", "save_probs=true"] + list(sys.argv[1:] if argv is None else argv))
    if not cfg.save_probs or cfg.synthetic != 1:
        raise SystemExit("[ivos-w] generate_data.py writes the probability planes of the synthetic back end: save_probs=true synthetic=1 are fixed")
    print(f"[ivos-w] generate_data: the synthetic back end (stand-in VOS model, synthetic sequences), save_probs=true -> {cfg.agent.save_result_dir}")
    _print_metric_mode(cfg)
    return run_eval(cfg, "MANet")


# ------------------------------------------------------------------------------------------ quality_assessment.py (the head fit)
# the reference's configs/config.yaml, assess_net section, and the keys this script adds (fit, zero_grad, augment_copies, val_fraction)
ASSESS_NET_DEFAULTS = dict(num_epochs=50, lr=5e-6, gamma=0.95, momentum=0.9, weight_decay=5e-4, train_batch_size=32, fit="head", zero_grad=True,
                           augment_copies=1, val_fraction=0.1)


def run_fit_head(cfg):
    """quality_assessment.py on this path: AssessNet's score head fitted to the back end's samples on the device (utils_agent.fit_assess_head).
    Writes <ckpt_dir>/assess_net.pt and <report_save_dir>/quality_assessment/{summary.json, head_fit_bank.npz}; returns the summary."""
    from .models.assessment import AssessNet
    from .utils import misc, utils_agent, utils_manet
    from . import synth
    a = cfg.assess_net
    if isinstance(a.get("lr"), str):                                   # a sweep: assess_net.lr=[1e-5,5e-6]
        try:
            a["lr"] = [float(v) for v in a["lr"].strip("[]()").split(",") if v.strip()]
        except ValueError:
            raise SystemExit(f"[ivos-w] assess_net.lr must be a number or a list like [1e-5,5e-6], got {a['lr']!r}")
    try:
        opts = utils_agent.head_fit_options(cfg)
    except ValueError as e:
        raise SystemExit(f"[ivos-w] {e}")
    if not torch.cuda.is_available():
        raise SystemExit("[ivos-w] the hot path needs an MI355X (no CPU fallback)")
    device = torch.device(f"cuda:{cfg.gpu_id}")
    print("[ivos-w] quality_assessment: no DAVIS frames and dumped samples on this path: the synthetic session and the stand-in VOS model "
          "supply them; assess_net.fit=head (fc1 on the pooled features of the frozen trunk)")
    misc.set_random_seed(int(cfg.seed))
    davis = SyntheticDavis(cfg, device)
    vos = StandInVOS(device, seed=int(cfg.seed))
    assess_net = AssessNet(precision=cfg.precision)
    ck = os.path.join(cfg.ckpt_dir, "assess_net.pt")
    if not misc.load_network_checkpoint(ck, assess_net, device="cpu"):
        print(f"[ivos-w] no {ck}: AssessNet starts from the seeded synthetic weights")
        assess_net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.assessnet_state_dict(0, spread=True).items()})
    assess_net = assess_net.to(device).eval()
    videos = []
    for seq, info in davis.dataset.items():                            # every sequence after its first interaction (frame 0 annotated)
        w, h = info["image_size"]
        store = utils_manet.ProbStore(info["num_frames"], info["num_objects"] + 1, h, w, device)
        _, all_P = _segment(vos, davis, seq, info["num_objects"], [0], store)
        videos.append((davis.load_frames(seq), davis.load_annotations(seq), all_P, info["num_objects"]))
    metric = cfg.davis_interactive.metric
    bank = {}
    fit = utils_agent.fit_assess_head(videos, assess_net, metric, cfg, seed=int(cfg.seed), bank_out=bank)
    res = fit["result"]
    for e in range(res.num_epochs):                                    # the reference's epoch line
        print(f"* Epoch: [{e:3d}]\tLoss: {res.epoch_loss[res.best, e]:.6f}\tdiff: {res.epoch_diff[res.best, e]:.6f}")
    misc.save_network_checkpoint(cfg.ckpt_dir, assess_net)
    report_dir = os.path.join(cfg.report_save_dir, "quality_assessment")
    os.makedirs(report_dir, exist_ok=True)
    np.savez(os.path.join(report_dir, "head_fit_bank.npz"), **{k: v for k, v in bank.items() if v is not None},
             epoch_loss=res.epoch_loss, epoch_diff=res.epoch_diff, log=res.log.cpu().numpy())
    chosen = {k: (float(v) if isinstance(v, float) else v) for k, v in fit["chosen"].items()}
    summary = {"fit": dict(before=fit["before"], after=fit["after"], holdout=fit["holdout"], chosen=chosen, metric=metric,
                           num_epochs=res.num_epochs, steps_per_epoch=res.steps_per_epoch, batch_size=res.batch_size,
                           epoch_loss=[float(v) for v in res.epoch_loss[res.best]], epoch_diff=[float(v) for v in res.epoch_diff[res.best]])}
    with open(os.path.join(report_dir, "summary.json"), "w") as fp:
        json.dump(summary, fp)
    print(f"# fit: loss {fit['before']['loss']:.6f} -> {fit['after']['loss']:.6f}  diff {fit['before']['diff']:.6f} -> {fit['after']['diff']:.6f}  "
          f"n {fit['after']['n']}  lr {chosen['lr']:g}  -> {os.path.join(cfg.ckpt_dir, 'assess_net.pt')}")
    summary["report_dir"] = report_dir
    return summary


def main_quality_assessment(argv=None):
    cfg = parse_cli(sys.argv[1:] if argv is None else argv, seed=2019, assess_net=dict(ASSESS_NET_DEFAULTS))     # the reference's set_random_seed(2019)
    return run_fit_head(cfg)


def main_train(argv=None):
    cfg = parse_cli(sys.argv[1:] if argv is None else argv, phase="train")
    _print_metric_mode(cfg)
    return run_train(cfg)
