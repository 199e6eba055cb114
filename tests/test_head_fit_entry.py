"""quality_assessment.py on the synthetic session with a tiny video: it writes the checkpoint and the ``fit`` block, logs the reference's
epoch line, and its per-epoch log equals what tests/head_fit_ref.py gives on the feature bank the run dumped, under the tolerance of
tests/test_gpu_head_fit.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ivos_w_amd  # noqa: F401
from ivos_w_amd import entry
from tests import head_fit_ref as R

pytestmark = pytest.mark.gpu


def test_quality_assessment_fits_the_head_on_the_synthetic_session(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ckpt, rep = str(tmp_path / "weights"), str(tmp_path / "results")
    summary = entry.main_quality_assessment(["with", "assess_net.num_epochs=2", "assess_net.augment_copies=1", "assess_net.train_batch_size=4",
                                             "assess_net.lr=1e-4", "precision=fp32", "synth.n_sequences=1", "synth.n_frames=6", "synth.height=64",
                                             "synth.width=96", f"ckpt_dir={ckpt}", f"report_save_dir={rep}"])
    text = capsys.readouterr().out
    assert "the synthetic session and the stand-in VOS model" in text and "zero_grad=true (plain SGD)" in text
    lines = re.findall(r"^\* Epoch: \[\s*(\d+)\]\tLoss: ([0-9.]+)\tdiff: ([0-9.]+)$", text, re.M)
    assert [int(e) for e, _, _ in lines] == [0, 1]
    assert os.path.exists(os.path.join(ckpt, "assess_net.pt"))
    on_disk = json.load(open(os.path.join(summary["report_dir"], "summary.json")))
    fit = on_disk["fit"]
    assert set(fit) >= {"before", "after", "chosen", "holdout"} and set(fit["before"]) == {"loss", "diff", "n"}
    assert fit["before"]["n"] == fit["after"]["n"] > 0 and fit["chosen"]["lr"] == 1e-4 and fit["num_epochs"] == 2
    assert fit["after"]["loss"] != fit["before"]["loss"]
    # the saved head is the fitted one
    sd = torch.load(os.path.join(ckpt, "assess_net.pt"), map_location="cpu")
    bank = np.load(os.path.join(summary["report_dir"], "head_fit_bank.npz"))
    # the run's log against the restatement on the dumped bank: the shuffles are fit_head's (RandomState(seed), full batches)
    M, Bsz, seed = bank["features"].shape[0], int(bank["batch_size"]), int(bank["seed"])
    held = np.zeros(M, bool)
    held[bank["holdout"]] = True
    rows = np.flatnonzero(~held)
    steps = len(rows) // Bsz
    rng = np.random.RandomState(seed)
    order = np.concatenate([rows[rng.permutation(len(rows))[:steps * Bsz]] for _ in range(2)]).astype(np.int32).reshape(2 * steps, Bsz)
    lr = R.lr_table(1e-4, 0.95, 2, steps)
    args = (bank["features"], bank["target"], bank["valid"], order, lr, 0.9, 5e-4, 1)
    l64, s64 = R.run(*args, 0, R.fresh_state(bank["w0"], float(bank["b0"])), np.float64)
    tl, tw, tb, _, _ = R.torch_loop(*args, bank["w0"], float(bank["b0"]))
    R.within(bank["log"][0], l64, tl, "entry log")
    R.within(sd["fc1.weight"].numpy().reshape(-1), s64["w"], tw, "entry w")
    R.within(sd["fc1.bias"].numpy().reshape(-1)[0], s64["b"], tb, "entry b")
    took = np.maximum((l64[:, 2] > 0).reshape(2, steps).sum(1), 1)
    want = l64[:, 0].reshape(2, steps).sum(1) / took
    t_ep = tl[:, 0].reshape(2, steps).sum(1) / took
    R.within(fit["epoch_loss"], want, t_ep, "entry epoch loss")
    np.testing.assert_allclose([float(v) for _, v, _ in lines], fit["epoch_loss"], atol=1e-6)
