#!/usr/bin/env python3
"""Train a MicrobeCensus model on the GPU: the reference's training/ workflow (TRAINING.txt steps 1 - 4, and step 5 with
--fit-weights) in one command.

    train_microbe_census.py <genomes_dir> <out_dir> -l 100,150 -c 10 [--gene-fams DIR] [-x 10] [--seed S] [-g device] [--write-reads DIR]
        [--error-model illumina|uniform [--error-rate R]] [--paired-end --insert I]
        [--fit-weights [--fit-seed S --fit-candidates C --fit-generations G]]

out_dir receives markers.faa.gz and model.json (use them with run_microbe_census.py --model out_dir) and the reference's tables
(pars.map, coefficients.map, weights.map, read_len.map, gene_fam.map, gene_len.map, training_preds.map)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbecensus_amd import training  # noqa: E402


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(usage="%s <genomes_dir> <out_dir> -l L[,L...] -c COV [-options]" % os.path.basename(__file__),
                                description="Simulate shotgun libraries of complete genomes, search and grid-classify them on the GPU, and fit "
                                            "the per-family mapping parameters and proportionality constants of an AGS model.")
    p.add_argument("genomes_dir", help="directory of complete genomes, one <name>.fna.gz per genome")
    p.add_argument("out_dir", help="directory for the model (markers.faa.gz, model.json) and the .map tables")
    p.add_argument("-l", dest="read_lengths", required=True, help="read lengths to train for, comma separated (18..510)")
    p.add_argument("-c", dest="coverage", type=float, required=True, help="library coverage of every genome (TRAINING.txt suggests 10)")
    p.add_argument("--gene-fams", dest="gene_fams", default=None, help="directory of marker gene families, one <family>.faa.gz each (default: the packaged markers)")
    p.add_argument("-x", dest="xfolds", type=int, default=10, help="folds of the cross-validation (default 10)")
    p.add_argument("--seed", dest="seed", type=int, default=0, help="seed of the read simulator (default 0)")
    p.add_argument("-g", dest="device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("--write-reads", dest="write_reads", default=None, help="also write every library as <DIR>/<L>/<genome>-reads.fa and its grid counts as <genome>.hits")
    p.add_argument("--error-model", dest="error_model", choices=training.ERROR_MODELS, default=None,
                   help="sequencing errors of the simulated reads (seq_sim.py -e; default: none)")
    p.add_argument("--error-rate", dest="error_rate", type=float, default=None, help="per-base error rate of --error-model uniform (seq_sim.py -r)")
    p.add_argument("--paired-end", dest="paired_end", action="store_true", help="simulate mate pairs (seq_sim.py -p): reads k/1 and k/2 of every fragment")
    p.add_argument("--reference-lengths", dest="reference_lengths", action="store_true",
                   help="reads of seq_sim.py's lengths, L + insertions - deletions (default: every read keeps L bases); rates over the real bp")
    p.add_argument("--insert", dest="insert", type=int, default=None, help="fragment length of --paired-end, at least the read length (seq_sim.py -i)")
    p.add_argument("--fit-weights", dest="fit_weights", action="store_true",
                   help="fit the per-family weights on the GPU (TRAINING.txt step 5; default: every weight 1.0)")
    p.add_argument("--fit-seed", dest="fit_seed", type=int, default=0, help="seed of the weight fit's candidates (default 0)")
    p.add_argument("--fit-candidates", dest="fit_candidates", type=int, default=None, help="candidates per generation of the weight fit (default: the library's)")
    p.add_argument("--fit-generations", dest="fit_generations", type=int, default=None, help="generations of the weight fit (default: the library's)")
    args = p.parse_args(argv)
    if not args.fit_weights and (args.fit_seed != 0 or args.fit_candidates is not None or args.fit_generations is not None):
        p.error("--fit-seed, --fit-candidates and --fit-generations go only with --fit-weights")
    try:
        args.read_lengths = [int(x) for x in args.read_lengths.split(",") if x.strip()]
    except ValueError:
        p.error("-l takes integers separated by commas")
    return args


def main(argv=None):
    a = parse_arguments(argv)
    try:
        training.train(a.genomes_dir, a.out_dir, a.read_lengths, a.coverage, gene_fams_dir=a.gene_fams, xfolds=a.xfolds, seed=a.seed,
                       device=a.device, write_reads_dir=a.write_reads, error_model=a.error_model, error_rate=a.error_rate,
                       paired_end=a.paired_end, insert=a.insert, reference_lengths=a.reference_lengths, fit_weights=a.fit_weights, fit_seed=a.fit_seed,
                       fit_candidates=a.fit_candidates, fit_generations=a.fit_generations)
    except training.TrainingError as e:
        sys.exit("Error: %s" % e)
    except RuntimeError as e:
        if not a.fit_weights:
            raise
        sys.exit("Error: %s" % e)


if __name__ == "__main__":
    main()
