#!/usr/bin/env python3
"""Gene abundances in RPKG (the reference README's "Normalization": reads mapped to gene / gene length in kb / genome equivalents)
from a metagenome and a protein FASTA of the user's genes, counted on the GPU.  The reads are sampled, filtered and trimmed by the
flags of scripts/run_microbe_census.py; the AGS is --ags, --ags-report, or the estimate of the same sample."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbecensus_amd import abundance, microbe_census  # noqa: E402


def parse_arguments(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--model", dest="model_dir", default=None)
    model_dir = pre.parse_known_args(argv)[0].model_dir
    if model_dir is not None:
        microbe_census.check_model_dir(model_dir)
    p = argparse.ArgumentParser(usage="%s [-options] <seqfiles> <genes.faa[.gz]> <out.tsv>" % os.path.basename(__file__),
                                description="Per-gene read counts and RPKG of a metagenome against a protein FASTA (GPU search and counting).")
    p.add_argument("seqfiles", type=str, help="path to input metagenome(s); comma separated; FASTA/FASTQ, optionally gz/bz2")
    p.add_argument("genes", type=str, help="protein FASTA of the genes (plain or .gz): at most 32,767 sequences of at most 2,047 residues")
    p.add_argument("outfile", type=str, help="path of the gene table (TSV)")
    p.add_argument("-v", dest="verbose", action="store_true", default=False, help="print the AGS estimate's progress to stdout")
    p.add_argument("-n", dest="nreads", type=int, default=2000000, help="number of reads to sample (default = 2000000)")
    p.add_argument("-t", dest="threads", type=int, default=None, help="cap on the host threads of the read sampler")
    p.add_argument("-l", dest="read_length", type=int, choices=microbe_census._valid_read_lengths(model_dir), help="trim all reads to this length")
    p.add_argument("-q", dest="min_quality", type=int, default=-5, help="minimum base-level PHRED quality (default = -5; no filtering)")
    p.add_argument("-m", dest="mean_quality", type=int, default=-5, help="minimum read-level PHRED quality (default = -5; no filtering)")
    p.add_argument("-d", dest="filter_dups", action="store_true", default=False, help="filter duplicate reads")
    p.add_argument("-u", dest="max_unknown", type=int, default=100, help="max percent of unknown bases per read (default = 100)")
    p.add_argument("-g", dest="device", type=int, default=None, help="GPU index (default: 0)")
    p.add_argument("--model", dest="model_dir", type=str, default=None, help="directory of a trained model for the AGS estimate instead of the packaged one")
    p.add_argument("--min-ident", dest="min_ident", type=int, default=0, metavar="P", help="count a read's alignments of at least P percent identity (an integer, 0 - 100; default = 0)")
    p.add_argument("--min-aln", dest="min_aln", type=int, default=0, metavar="A", help="... of at least A aligned residues (default = 0)")
    p.add_argument("--min-bits", dest="min_bits", type=float, default=0.0, metavar="S", help="... of a bit score of at least S (default = 0)")
    p.add_argument("--groups", dest="groups", type=str, default=None, metavar="map.tsv", help="TSV of gene and group: adds <out>.groups.tsv with the groups' sums")
    p.add_argument("--ags", dest="ags", type=float, default=None, metavar="VALUE", help="average genome size in bp to normalise by")
    p.add_argument("--ags-report", dest="ags_report", type=str, default=None, metavar="FILE", help="report of run_microbe_census.py (or of the reference) to take the average genome size from")
    p.add_argument("--coverage", dest="coverage", action="store_true", default=False, help="add covered_aa, breadth (covered_aa / length_aa), mean_depth and max_depth: which part of a gene its reads cover")
    p.add_argument("--min-breadth", dest="min_breadth", type=float, default=None, metavar="F", help="add the column detected: reads > 0 and breadth >= F (0 < F <= 1); implies --coverage")
    p.add_argument("--depth-out", dest="depth_out", type=str, default=None, metavar="FILE", help="write the per-residue depth as gene, start, end, depth (0-based start, exclusive end); implies --coverage")
    p.add_argument("--ties", dest="ties", action="store_true", default=False, help="add unique_reads, candidate_reads, shared_reads and rpkg_shared: the genes that tie for a read's highest bit score share the read "
                   "(with --coverage also covered_any_aa and breadth_any, with --min-breadth detected_any, with --groups the groups' unique and shared reads)")
    p.add_argument("--curve", dest="curve", type=int, default=None, metavar="K", help="a rarefaction curve: the table's figures at K nested prefixes of the sample (1 - 64), as runs with -n n_k would give them; "
                   "writes <out>.curve.tsv.  The reads are sampled to the end before the search starts; the tie columns are not rarefied")
    p.add_argument("--curve-genes", dest="curve_genes", type=str, default=None, metavar="FILE", help="with --curve: write the per-gene matrix, gene, reads_1 .. reads_K (and covered_aa_1 .. covered_aa_K with coverage)")
    p.add_argument("--bootstrap", dest="bootstrap", type=int, default=None, metavar="B", help="add rpkg_boot_se, rpkg_ci95_low and rpkg_ci95_high: the standard error and 95%% interval of every RPKG from B Poisson-bootstrap "
                   "replicates of the sampled reads (1 - 4096); with the default AGS every replicate is divided by its own AGS estimate, with --ags / --ags-report by the given one.  Not combined with --curve")
    p.add_argument("--bootstrap-seed", dest="bootstrap_seed", type=int, default=None, metavar="S", help="with --bootstrap: the seed of the replicates (default = 0)")
    p.add_argument("--bootstrap-groups", dest="bootstrap_groups", action="store_true", default=False,
                   help="with --bootstrap and --groups: add rpkg_boot_se, rpkg_ci95_low and rpkg_ci95_high to <out>.groups.tsv, from the same replicates summed over every group's genes "
                        "(a group's error bar does not follow from its members': their replicates are correlated)")
    p.add_argument("--bootstrap-ties", dest="bootstrap_ties", action="store_true", default=False,
                   help="with --bootstrap and --ties: add rpkg_shared_boot_se, rpkg_shared_ci95_low and rpkg_shared_ci95_high behind every column of the gene table, from the same replicates "
                        "on every gene's even share of the reads it ties for (the error bar of a single allele, variant or family member)")
    p.add_argument("--tie-list-factor", dest="tie_list_factor", type=int, default=None, metavar="F",
                   help="with --bootstrap-ties: the device keeps one entry per read and tied gene in a list of F times the sampled reads, at most 2^27 entries (1 - 500; default = 4); "
                        "a run whose tied sets do not fit is refused and names the F that fits")
    p.add_argument("--bootstrap-coverage", dest="bootstrap_coverage", action="store_true", default=False,
                   help="with --bootstrap and --coverage, --min-breadth or --depth-out: add breadth_boot_mean, breadth_boot_se, breadth_ci95_low and breadth_ci95_high behind every column of "
                        "the gene table and, with --min-breadth, detected_support: the share of the replicates in which the gene is detected (how much breadth and the detection call hang on "
                        "single reads; the interval lies at or below breadth)")
    p.add_argument("--mixed-lengths", dest="mixed_lengths", nargs="?", const=True, default=None, metavar="L1,L2,...",
                   type=lambda v: [int(x) for x in v.split(",")],
                   help="count every read at the largest of the model's read lengths it reaches, instead of cutting all reads to one length and dropping the shorter ones; "
                        "the genome equivalents are those of the bases so sampled.  The optional list names the length classes (default: the length_classes line of --ags-report, "
                        "else the model's lengths that at least 1%% of the first 10,000 reads fall in).  Not combined with -l and --curve; --bootstrap under it needs --ags or --ags-report")
    p.add_argument("--long-genes", dest="long_genes", action="store_true", default=False,
                   help="accept genes of up to 65,535 residues: a gene longer than the engine's longest sequence is searched as overlapping segments and every table "
                        "reports the whole gene; adds long_genes, genes_split, segments and edge_rows to the header")
    p.add_argument("--identity", dest="identity", action="store_true", default=False,
                   help="add matched_aa, mismatched_aa, gap_opens, ident_mean, ident_median, ident_min and ident_max behind every column of the gene table: how similar the reads "
                        "assigned to a gene are to its sequence (percent identity of every read's best row; with --groups matched_aa and ident_mean in <out>.groups.tsv)")
    p.add_argument("--ident-levels", dest="ident_levels", default=None, metavar="T1,T2,...", type=lambda v: [int(x) for x in v.split(",")],
                   help="per level T add reads_ident_ge<T> and rpkg_ident_ge<T>: the reads whose BEST ROW has at least T percent identity (1 - 8 integers, 0 - 100, ascending); "
                        "not the reads of a run with --min-ident T, where a lower-scoring row of higher identity may win; implies --identity")
    p.add_argument("--ident-out", dest="ident_out", type=str, default=None, metavar="FILE", help="write the identity histogram as gene, ident, reads: one line per gene and percent that has reads; implies --identity")
    p.add_argument("--depth-stats", dest="depth_stats", action="store_true", default=False,
                   help="add median_depth, tad<P> and tad<P>_per_ge behind every column of the gene table: the lower median and the truncated average of the per-residue depth "
                        "(zeros included), which a pile of reads on one conserved domain does not move, and that average per genome equivalent - roughly the gene's copies per "
                        "genome, biased low (with --ties also median_depth_any and tad<P>_any); implies --coverage")
    p.add_argument("--tad-keep", dest="tad_keep", type=int, default=None, metavar="P",
                   help="the percent of the sorted depths the truncated average keeps, (100 - P) / 2 percent cut at either end (an integer, 1 - 100; default = 80: tad80); implies --depth-stats")
    args = vars(p.parse_args(argv))
    args["seqfiles"] = args["seqfiles"].split(",")
    for k in ("device", "model_dir", "threads"):
        if args[k] is None:
            del args[k]
    return args


if __name__ == "__main__":
    try:
        table, args = abundance.run_abundance(parse_arguments())
    except abundance.AbundanceError as e:
        sys.exit("Error! %s" % e)
    print("%d of %d sampled reads assigned to %d of %d genes; table: %s" % (table["reads_assigned"], table["sampled_reads"], int((table["reads"] > 0).sum()),
                                                                           len(table["gene"]), args["outfile"]))
