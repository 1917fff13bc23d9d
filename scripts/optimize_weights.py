#!/usr/bin/env python3
"""Fit the per-family weights of a trained model on the GPU: the reference's training step 5 (optimize_weights.R) as a command.

    optimize_weights.py <model_dir> [-g device] [--fit-seed S] [--fit-candidates C] [--fit-generations G]

Reads <model_dir>/training_preds.map (written by train_microbe_census.py), fits one weight per (read length, family) and rewrites
weights.map and the weights of model.json - the weights train_microbe_census.py --fit-weights writes with the same settings."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbecensus_amd import training  # noqa: E402


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(usage="%s <model_dir> [-options]" % os.path.basename(__file__),
                                description="Fit the per-family weights of a trained AGS model on the GPU (TRAINING.txt step 5).")
    p.add_argument("model_dir", help="model directory written by train_microbe_census.py (holds training_preds.map)")
    p.add_argument("-g", dest="device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("--fit-seed", dest="fit_seed", type=int, default=0, help="seed of the candidates (default 0)")
    p.add_argument("--fit-candidates", dest="fit_candidates", type=int, default=None, help="candidates per generation (default: the library's)")
    p.add_argument("--fit-generations", dest="fit_generations", type=int, default=None, help="generations (default: the library's)")
    return p.parse_args(argv)


def main(argv=None):
    a = parse_arguments(argv)
    try:
        training.refit_model_dir(a.model_dir, device=a.device, seed=a.fit_seed, candidates=a.fit_candidates, generations=a.fit_generations)
    except (training.TrainingError, RuntimeError) as e:
        sys.exit("Error: %s" % e)


if __name__ == "__main__":
    main()
