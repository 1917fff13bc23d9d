#!/usr/bin/env python3
"""Score a MicrobeCensus model on mock communities of known composition: simulated metagenomes made and searched on the GPU, the AGS
estimate of each against the exact truth.

    validate_microbe_census.py <genomes_dir> <out_dir> [--model DIR] [--communities FILE.tsv ... | --random K --members M --sigma S]
        -l 100,150 -n 2000000 [--seed S] [-g device] [--error-model illumina|uniform [--error-rate R]] [--paired-end --insert I] [--write-reads DIR]

A community file is a TSV with a header line: the first column names the genome (<name>.fna.gz in genomes_dir), the column headed
relative_abundance (or abundance) gives its share of the cells.  out_dir receives validation.map (community, read_length, members,
reads, true_ags, est_ags, error; then per read length the median and maximum unsigned error) and communities/<name>.tsv (genome,
copies, size, reads drawn)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbecensus_amd import training, validation  # noqa: E402


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(usage="%s <genomes_dir> <out_dir> -l L[,L...] -n READS [-options]" % os.path.basename(__file__),
                                description="Simulate metagenomes of mock communities on the GPU, estimate their average genome size with a model "
                                            "and report the error against the communities' true AGS.")
    p.add_argument("genomes_dir", help="directory of complete genomes, one <name>.fna.gz per genome")
    p.add_argument("out_dir", help="directory for validation.map and communities/<name>.tsv")
    p.add_argument("--model", dest="model_dir", default=None, help="model directory written by train_microbe_census.py (default: the packaged model)")
    p.add_argument("--communities", dest="communities", nargs="+", default=None, help="community files (TSV: genome, relative_abundance)")
    p.add_argument("--random", dest="random", type=int, default=0, help="number of random communities")
    p.add_argument("--members", dest="members", type=int, default=None, help="genomes per random community")
    p.add_argument("--sigma", dest="sigma", type=float, default=1.0, help="sigma of the random communities' log-normal abundances (default 1)")
    p.add_argument("-l", dest="read_lengths", default="", help="read lengths, comma separated (ones the model was trained for)")
    p.add_argument("--length-mix", dest="length_mix", default=None, metavar="L1:s1,L2:s2,...",
                   help="also score libraries of mixed lengths, e.g. 100:0.5,150:0.5: per community one pass per length with round(share x n) reads, "
                        "combined as run_microbe_census.py --mixed-lengths combines them (validation.map rows with read_length 100+150)")
    p.add_argument("-n", dest="nreads", type=int, required=True, help="reads per simulated metagenome")
    p.add_argument("--seed", dest="seed", type=int, default=0, help="seed of the communities and of the read simulator (default 0)")
    p.add_argument("-g", dest="device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("--error-model", dest="error_model", choices=training.ERROR_MODELS, default=None, help="sequencing errors of the simulated reads (default: none)")
    p.add_argument("--error-rate", dest="error_rate", type=float, default=None, help="per-base error rate of --error-model uniform")
    p.add_argument("--paired-end", dest="paired_end", action="store_true", help="simulate mate pairs: reads k/1 and k/2 of every fragment")
    p.add_argument("--insert", dest="insert", type=int, default=None, help="fragment length of --paired-end, at least the read length")
    p.add_argument("--reference-lengths", dest="reference_lengths", action="store_true", help="refused: a community library has reads of one length")
    p.add_argument("--write-reads", dest="write_reads", default=None, help="also write every metagenome as <DIR>/<community>_<L>.fa.gz")
    args = p.parse_args(argv)
    try:
        args.read_lengths = [int(x) for x in args.read_lengths.split(",") if x.strip()]
    except ValueError:
        p.error("-l takes integers separated by commas")
    if not args.read_lengths and not args.length_mix:
        p.error("give -l, --length-mix or both")
    if args.length_mix:
        try:
            args.length_mix = validation.parse_length_mix(args.length_mix)
        except validation.ValidationError as e:
            p.error(str(e))
    if args.communities and args.random:
        p.error("--communities and --random exclude each other")
    return args


def main(argv=None):
    a = parse_arguments(argv)
    try:
        validation.validate(a.genomes_dir, a.out_dir, a.read_lengths, a.nreads, model_dir=a.model_dir, communities=a.communities, random=a.random,
                            members=a.members, sigma=a.sigma, seed=a.seed, device=a.device, error_model=a.error_model, error_rate=a.error_rate,
                            paired_end=a.paired_end, insert=a.insert, write_reads_dir=a.write_reads, reference_lengths=a.reference_lengths,
                            length_mix=a.length_mix)
    except (validation.ValidationError, training.TrainingError) as e:
        sys.exit("Error: %s" % e)


if __name__ == "__main__":
    main()
