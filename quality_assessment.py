#!/usr/bin/env python
"""quality_assessment.py — fits AssessNet's score head to the samples of a VOS back end, on the device.

    python quality_assessment.py with [assess_net.num_epochs=50] [assess_net.lr=5e-6 | assess_net.lr=[1e-5,5e-6]] [key=value ...]

The reference's entry point of this name trains the whole AssessNet.  On this path the trunk runs with folded BatchNorm, so it is frozen
and fc1 (2048 -> 1) is fitted on its pooled features with the reference's optimiser loop (clamped gradients, SGD with momentum and weight
decay, ExponentialLR): assess_net.fit=head, the only accepted value.  Defaults are the reference's configs/config.yaml; new keys:
assess_net.zero_grad (false = the reference's accumulating gradients), assess_net.augment_copies, assess_net.val_fraction; a list in
assess_net.lr is a sweep (the lowest held-out loss wins).  Without DAVIS and dumped samples it says so and uses the synthetic session
(see ivos-w_amd/entry.py: run_fit_head).  Writes <ckpt_dir>/assess_net.pt and a "fit" block in <report_save_dir>/quality_assessment/summary.json.
"""
import ivos_w_amd  # noqa: F401  (registers the package under its importable name)
from ivos_w_amd import entry

if __name__ == "__main__":
    entry.main_quality_assessment()
