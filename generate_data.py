#!/usr/bin/env python
"""generate_data.py — writes AssessNet's training samples: the probability maps of every interaction as 8-bit planes.

    python generate_data.py with setting=wild method=ours [agent.save_result_dir=train] [key=value ...]

The reference's entry point of this name runs the MANet evaluation loop and saves all_P after every interaction (save_seg_preds).  Here
the same loop runs on the synthetic back end with save_probs=true (it says so on stdout): the planes are quantised on the device and
written under <agent.save_result_dir>/interaction-{n}/scribble-{s}/{sequence}/probs/{obj}/{frame:05d}.png (see ivos-w_amd/entry.py).
"""
import ivos_w_amd  # noqa: F401  (registers the package under its importable name)
from ivos_w_amd import entry

if __name__ == "__main__":
    entry.main_generate()
