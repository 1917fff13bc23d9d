"""Gene abundances in RPKG - the use the reference's README gives for genome equivalents (section "Normalization"):

    RPKG = (reads mapped to gene) / (gene length in kb) / (genome equivalents)

The reads are sampled, filtered and trimmed exactly as run_pipeline does it (same reader, same -n -l -q -m -d -u), searched
against the user's protein FASTA on the GPU, and counted per gene ON the device (Engine.set_abundance; csrc/k_abundance.h states
the rule): no m8 row reaches the host.  Numerator and denominator come from the SAME sampled bases:

    genome_equivalents_sampled = sampled_reads x trimmed_length / AGS          (the file's total bases are not used)
    rpkg = reads / (3 x length_aa / 1000) / genome_equivalents_sampled

The AGS is --ags VALUE, the average_genome_size line of a report (--ags-report FILE), or - by default - run_pipeline on the same
files with the same options in the same process (the marker engine; the gene engine is a second Engine on the same device).

A high RPKG alone does not say that a gene is there: a few hundred reads piled on one conserved domain give one.  With coverage
(Engine.set_coverage; csrc/k_coverage.h states the rule) the table also says which part of the gene the assigned reads cover: a best
row covers the subject residues sstart .. send of RAPsearch2's m8 - 0-based and inclusive - and per gene

    covered_aa = residues covered by at least one read      breadth = covered_aa / length_aa
    mean_depth = (sum of the depths) / length_aa            max_depth = the largest depth

min_breadth F adds the column detected (reads > 0 and covered_aa >= F x length_aa); depth_out writes the depth itself, run-length
encoded (gene, start, end, depth: 0-based start, exclusive end).

The counts give a read to ONE gene: the first row of its highest bit score.  Among near-identical genes - alleles, variants, families -
most reads tie, and the first of the tied genes gets them all.  With ties (Engine.set_ties; csrc/k_ties.h states the rule) the table
also says, per gene, how many of its reads were its alone, how many it tied for, and what an even split gives it:

    unique_reads    = reads whose highest bit score only this gene has      candidate_reads = reads that have it on this gene
    shared_reads    = the sum over those reads of 1 / k, k the genes tied   rpkg_shared     = the rpkg formula on shared_reads

and with coverage covered_any_aa / breadth_any (the residues that a tied read covers, whichever gene it was given to) and, with
min_breadth, detected_any (candidate_reads > 0 and covered_any_aa >= F x length_aa).  The existing columns keep their values.

Was the sample sequenced deeply enough?  With curve K (Engine.set_curve; csrc/k_curve.h states the rule) the same run also gives every
figure the table is built from at K nested prefixes of the sample, n_k = microbe_census.curve_points(sampled_reads, K) - the points of
run_pipeline's AGS curve: reads, aligned_aa and covered_aa per gene and, from them by the lines above, RPKG, reads_assigned, the genes
with reads, the genes detected and the groups with reads.  The sampler is a head-take, so point k is, integer for integer, the table
of a run with -n n_k, and the last point is the run's own table.  The tie columns stay whole-sample figures: the curve does not
rarefy them.

How sure is an RPKG?  With bootstrap B (Engine.set_gene_bootstrap; csrc/mc_geneboot.h states the rule) the sampled reads are resampled B
times with Poisson(1) weights - the weights of run_pipeline's AGS bootstrap, a pure function of (seed, replicate, read id) - and replicate
b of the gene counts is divided by replicate b of the genome equivalents: numerator and denominator from the SAME resample.  Per gene

    rpkg_boot_se = the standard deviation (ddof 1) of the replicate RPKGs     rpkg_ci95_low / _high = their 2.5th / 97.5th percentile

With a given AGS (--ags, --ags-report) the denominator is fixed and the interval reflects the counts alone.

And how sure is a group's?  Not by its members' columns: a group's RPKG is the sum of theirs, their replicates are correlated - the genome
equivalents of replicate b divide all of them, and alleles that compete for the same reads move against each other - so neither the standard
error nor a percentile of the sum follows from the members'.  With bootstrap_groups (Engine.group_bootstrap; csrc/mc_groupboot.h states the
rule) replicate b of a group is the sum of its members' replicate RPKGs, added on the device in FASTA order, and the groups table gets the same
three columns from those sums.  It is also the level at which the bootstrap is most trustworthy: without ties a read that ties between alleles
goes to whichever row comes first, and tying alleles normally share a group.  The groups' tie columns stay whole-sample figures.

And a single allele's, variant's or family member's?  The figure to trust there is rpkg_shared, the column that splits a tied read evenly.  With
bootstrap_ties (Engine.set_tie_bootstrap; csrc/mc_tieboot.h states the rule; needs bootstrap and ties) replicate b of a gene's shared reads is
the sum over the reads it ties for of weight(b, read) x 1 / k - the same weights, so the same resample as replicate b of the counts and of the
genome equivalents - and the gene table gets rpkg_shared_boot_se, rpkg_shared_ci95_low and rpkg_shared_ci95_high behind every other column.  The
device keeps one entry per (read, tied gene) in a list of tie_list_factor (default 4, 1 .. 500) times the gene bootstrap's list, at most 2^27
entries; a run whose tied sets do not fit is refused and told the factor that fits.  For a gene none of whose reads tie the three columns are
rpkg's, bit for bit.  candidate_reads, unique_reads, the any-coverage columns and the groups table's tie columns are not bootstrapped.

How sure is `detected`?  breadth and detected are the most fragile figures of the table: three reads that happen to tile a gene lift it over
min_breadth exactly like a gene covered ten deep.  With bootstrap_coverage (Engine.set_coverage_bootstrap; csrc/mc_covboot.h states the rule;
needs bootstrap and coverage) replicate b of a gene's covered residues is what the best rows of the reads PRESENT in replicate b - weight(b,
read) > 0, the same resample as replicate b of the counts - cover, and the gene table gets breadth_boot_mean, breadth_boot_se, breadth_ci95_low
and breadth_ci95_high behind every other column and, with min_breadth, detected_support: the share of the B replicates that detect the gene.  A
Poisson(1) resample leaves out about 37 % of the reads, so covered_b <= covered_aa in every replicate and the interval lies at or below
breadth: it is no confidence interval of the true breadth but a measure of how much the figure hangs on single reads.  covered_any_aa,
detected_any, mean_depth, max_depth, the depth file and the groups table's genes_detected are not bootstrapped.

Reads of mixed lengths (mixed_lengths; README "Reads of mixed lengths"): one trimmed length drops every shorter read and the tail of
every longer one.  Under the switch every read is searched and counted at the largest length class L_k it reaches
(Engine.set_abundance_classes; csrc/k_abund_classes.h states the rule), and the denominator is that of the bases so sampled:

    sampled_bases = sum over the classes of n_k x L_k       genome_equivalents_sampled = sampled_bases / AGS

n_k the reads of class k, counted on the device beside the reads each class assigned.  The default AGS is run_pipeline's estimate
under the same classes: numerator and denominator still come from the same sampled bases.

How close is the gene to the database's?  A gene covered over 90 % of its length at 99 % identity is that allele; the same breadth at 65 % is a
distant homolog.  With identity (Engine.set_identity; csrc/mc_identity.h states the rule) the device also keeps, per gene, a histogram of the
floor of the identity in percent of every assigned read's BEST ROW - 100 x nmatch / alnlen, the row the counts take - and the sums of those
rows' identical, mismatched and gap-opening columns, and the gene table gets, behind every other column,

    matched_aa, mismatched_aa, gap_opens     ident_mean = 100 x matched_aa / aligned_aa     ident_median (the lower one), ident_min, ident_max

and per level T of ident_levels reads_ident_ge<T> - the reads whose best row has an identity of at least T percent - and rpkg_ident_ge<T>, the
rpkg formula on them.  That is NOT the reads column of a run with min_ident T: there a lower-scoring row of higher identity may win a read
whose best row fails the cut-off; the two agree for a read with one row.  ident_out writes the histogram (gene, ident, reads: one line per
non-empty bin).  The figures are whole-sample figures of the best row: not rarefied, not bootstrapped, not shared among tied genes.

Is the gene there, and how many copies?  reads, rpkg, mean_depth and max_depth all rise when a few hundred reads pile on one conserved domain.
With depth_stats (Engine.depth_stats; csrc/mc_depthstats.h states the rule; implies coverage) the device selects, per gene, order statistics
of the per-residue depth - zeros included, nothing sorted, no residue's depth copied out - and the gene table gets, behind every other column,

    median_depth (the lower median)     tad<P> = trimmed_sum / (hi - lo)     tad<P>_per_ge = tad<P> / genome_equivalents_sampled

where P is tad_keep (an integer percent, 1 .. 100, default 80; it implies depth_stats), cut = length_aa x (100 - P) // 200, lo = cut, hi =
length_aa - cut and trimmed_sum the sum of the sorted depths at the ranks lo .. hi - 1: the "truncated average depth", TAD80 at the default.
Neither moves when a domain is piled on; both are 0 for a gene covered over less than half (the median) or less than cut residues short of
all (tad) of its length.  With ties median_depth_any and tad<P>_any follow, from the any-depth.  tad<P>_per_ge is roughly the gene's copies per
genome - a single-copy gene present in every cell has a depth of about genome_equivalents_sampled - and it is biased LOW: reads that overlap a
gene's end too shortly to align, and reads that failed the cut-offs, are missing from the depth.  Whole-sample figures: not rarefied, not
bootstrapped, not summed into the groups table (a group has no depth)."""
import gzip
import math
import os
import re

import numpy as np

from . import _native, microbe_census

MAX_GENES = 32767         # MC_POST8 (csrc/mc_core.h): the engine's limits on a protein database
MAX_GENE_LEN = 2047


def _fold_define(name):
    """an integer constant of csrc/mc_fold.h: the rule of long genes is stated there once, and the library compiles that text"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_fold.h")) as f:
        return int(re.search(r"^#define %s (\d+)\b" % name, f.read(), re.M).group(1))


SEG_LEN = _fold_define("MC_FOLD_SEG_LEN")                 # long genes (long_genes; csrc/mc_fold.h): the longest sequence the engine opens,
SEG_OVERLAP = _fold_define("MC_FOLD_OVERLAP")         # what consecutive segments of a longer gene share,
MAX_LONG_GENE_LEN = _fold_define("MC_FOLD_MAX_GENE")   # and the gene-space limits
MAX_SEGMENTS = _fold_define("MC_FOLD_MAX_SEGS")

COLUMNS = ("gene", "length_aa", "reads", "aligned_aa", "rpkg")
GROUP_COLUMNS = ("group", "genes", "reads", "rpkg")
COVERAGE_COLUMNS = ("covered_aa", "breadth", "mean_depth", "max_depth")     # behind COLUMNS with coverage; "detected" behind them with min_breadth
DEPTH_COLUMNS = ("gene", "start", "end", "depth")
TIES_COLUMNS = ("unique_reads", "candidate_reads", "shared_reads", "rpkg_shared")    # behind all of them with ties ...
TIES_COVERAGE_COLUMNS = ("covered_any_aa", "breadth_any")                            # ... these behind them with coverage, "detected_any" last with min_breadth
GROUP_TIES_COLUMNS = ("unique_reads", "shared_reads", "rpkg_shared")                 # behind the groups table's columns; "genes_detected_any" last with min_breadth
CURVE_COLUMNS = ("sampled_reads", "average_genome_size", "genome_equivalents_sampled", "reads_assigned", "genes_with_reads")   # "genes_detected" behind them with min_breadth, "groups_with_reads" with groups
TIE_BOOT_COLUMNS = ("rpkg_shared_boot_se", "rpkg_shared_ci95_low", "rpkg_shared_ci95_high")   # behind every other column with bootstrap_ties
MAX_TIE_LIST = 1 << 27                                                               # MC_TB_MAXCAP (csrc/mc_tieboot.h): the most entries the tie list holds
MAX_TIE_FACTOR = 500                                                                 # MC_MAX_M8 (csrc/mc_core.h): no read ties across more genes
TIE_FACTOR = 4                                                                       # tie_list_factor's default
COV_BOOT_COLUMNS = ("breadth_boot_mean", "breadth_boot_se", "breadth_ci95_low", "breadth_ci95_high")   # behind those with bootstrap_coverage; "detected_support" last with min_breadth
BOOT_COLUMNS = ("rpkg_boot_se", "rpkg_ci95_low", "rpkg_ci95_high")                  # behind all of them with bootstrap; behind the groups table's with bootstrap_groups
MAX_BOOT = 4096                                                                      # MC_GB_MAXB (csrc/mc_geneboot.h)
MAX_CURVE = 64                                                                       # MC_CURVE_MAXK (csrc/mc_curve.h)
IDENT_COLUMNS = ("matched_aa", "mismatched_aa", "gap_opens", "ident_mean", "ident_median", "ident_min", "ident_max")   # behind every other column with identity; reads_ident_ge<T>, rpkg_ident_ge<T> per level behind them
IDENT_OUT_COLUMNS = ("gene", "ident", "reads")
IDENT_BINS = 101                                                                     # MC_ID_BINS (csrc/mc_identity.h)
MAX_IDENT_LEVELS = 8                                                                 # MC_ID_LEVELS
TAD_KEEP = 80                                                                        # tad_keep's default: the central 80 % of the sorted depths ("TAD80")
PIPELINE_KEYS = ("seqfiles", "nreads", "read_length", "min_quality", "mean_quality", "filter_dups", "max_unknown", "threads", "device", "model_dir", "verbose")
TEXT = {"s": str, "d": lambda v: "%d" % v, "f": lambda v: repr(float(v)), "n": lambda v: "NA" if v is None else repr(float(v)),
        "i": lambda v: "NA" if v is None else "%d" % v}   # a value in a table, by its column's kind
SHARE_ONE = 4294967296.0                                                             # share[] counts in units of 2^-32 (csrc/k_ties.h)


class AbundanceError(Exception):
    """What run_abundance refuses - before any GPU work."""


def read_genes(path, long_genes=False):
    """(names, seqs) of a protein FASTA (plain or .gz): a gene's name is the header's first token.  Refused: an empty FASTA, more than
    32,767 sequences, a sequence of more than 2,047 residues (with long_genes: of more than 65,535) or of none, duplicate names."""
    if not os.path.isfile(path):
        raise AbundanceError("Gene FASTA %s not found" % path)
    names, seqs = _native.load_markers(path) if not _starts_headless(path) else ([], [])
    if not names:
        raise AbundanceError("Gene FASTA %s is empty: it holds no sequence" % path)
    if len(names) > MAX_GENES:
        raise AbundanceError("Gene FASTA %s holds %d sequences: more than %d" % (path, len(names), MAX_GENES))
    seen = set()
    for nm, sq in zip(names, seqs):
        if nm in seen:
            raise AbundanceError("Gene name %s occurs more than once in %s" % (nm, path))
        seen.add(nm)
        if long_genes and len(sq) > MAX_LONG_GENE_LEN:
            raise AbundanceError("Gene %s is %d residues long: longer than %d, the limit of --long-genes" % (nm, len(sq), MAX_LONG_GENE_LEN))
        if not long_genes and len(sq) > MAX_GENE_LEN:
            raise AbundanceError("Gene %s is %d residues long: longer than %d (--long-genes searches a long gene as overlapping segments)" % (nm, len(sq), MAX_GENE_LEN))
        if len(sq) == 0:
            raise AbundanceError("Gene %s has no residues" % nm)
    return names, seqs


def segment_offsets(length, seg_len, overlap):
    """The offsets of the segments of a gene of `length` residues (csrc/mc_fold.h, "the segments"): one at 0 for a gene of at most
    seg_len residues, otherwise j * (seg_len - overlap) for j = 0, 1, .. up to the first segment that reaches the gene's end."""
    step = seg_len - overlap
    n = 1 if length <= seg_len else 1 + -(-(length - seg_len) // step)
    return [j * step for j in range(n)]


def split_genes(names, seqs, seg_len=SEG_LEN, overlap=SEG_OVERLAP):
    """The genes as the engine takes them under long_genes (csrc/mc_fold.h states the rule): every gene of more than seg_len residues
    cut into segments of seg_len that overlap by `overlap`, every other gene as it is.  Returns a dict: seg_names and seg_seqs (the
    database to open - a segment is named <gene>|<offset>, a gene of one segment keeps its name), seg_gene, seg_off (int32 per
    segment) and gene_len (int32 per gene) - the three maps of Engine.set_gene_fold -, stats (residues, sequences of the GENES: the
    database the alignment statistics are those of, Engine(stats=)), and genes_split.  Refused, naming the value: a gene of more than
    65,535 residues, and the gene at which the segments pass 32,767."""
    if not 0 <= overlap < seg_len:
        raise AbundanceError("An overlap of %d residues does not fit segments of %d" % (overlap, seg_len))
    seg_names, seg_seqs, seg_gene, seg_off, split = [], [], [], [], 0
    for g, (nm, sq) in enumerate(zip(names, seqs)):
        if len(sq) > MAX_LONG_GENE_LEN:
            raise AbundanceError("Gene %s is %d residues long: longer than %d, the limit of --long-genes" % (nm, len(sq), MAX_LONG_GENE_LEN))
        offs = segment_offsets(len(sq), seg_len, overlap)
        if len(seg_names) + len(offs) > MAX_SEGMENTS:
            raise AbundanceError("Gene %s (%d residues, %d segments) takes the database past %d segments: %d before it" % (nm, len(sq), len(offs), MAX_SEGMENTS, len(seg_names)))
        split += len(offs) > 1
        for o in offs:
            seg_names.append(nm if len(offs) == 1 else "%s|%d" % (nm, o))
            seg_seqs.append(sq[o:o + seg_len])
            seg_gene.append(g)
            seg_off.append(o)
    return {"seg_names": seg_names, "seg_seqs": seg_seqs, "seg_gene": np.array(seg_gene, np.int32), "seg_off": np.array(seg_off, np.int32),
            "gene_len": np.array([len(s) for s in seqs], np.int32), "stats": (sum(len(s) for s in seqs), len(seqs)), "genes_split": int(split)}


def _starts_headless(path):
    """True when the first non-empty line of the file is no FASTA header (load_markers would index a list that is not there)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        for line in f:
            if line.strip():
                return not line.startswith(">")
    return True


def read_groups(path, names):
    """{gene: group} of a TSV of gene and group (lines starting with # and empty lines skipped).  A gene that is not in the FASTA, or
    that is given two groups, is refused."""
    known = set(names)
    out = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.split("\t")
            if len(cols) < 2 or not cols[0] or not cols[1]:
                raise AbundanceError("%s line %d: expected gene<TAB>group, found %r" % (path, ln, line))
            gene, group = cols[0], cols[1]
            if gene not in known:
                raise AbundanceError("%s line %d: gene %s is not in the gene FASTA" % (path, ln, gene))
            if out.get(gene, group) != group:
                raise AbundanceError("%s line %d: gene %s is given two groups, %s and %s" % (path, ln, gene, out[gene], group))
            out[gene] = group
    return out


def read_ags_report(path):
    """The average_genome_size of a report written by report_results (this project's or the reference's: `average_genome_size:\\t<v>`)."""
    if not os.path.isfile(path):
        raise AbundanceError("AGS report %s not found" % path)
    with open(path) as f:
        for line in f:
            if line.startswith("average_genome_size:"):
                txt = line.split(":", 1)[1].strip()
                try:
                    return float(txt)
                except ValueError:
                    raise AbundanceError("AGS report %s: average_genome_size %r is not a number" % (path, txt))
    raise AbundanceError("AGS report %s has no average_genome_size line" % path)


def check_ags(ags, source):
    try:
        v = float(ags)
    except (TypeError, ValueError):
        raise AbundanceError("The AGS %r (%s) is not a number" % (ags, source))
    if not math.isfinite(v) or v <= 0:
        raise AbundanceError("The AGS %r (%s) is not a positive finite number" % (ags, source))
    return v


def genome_equivalents(sampled_reads, read_length, ags):
    return sampled_reads * read_length / ags


def sampled_bases(class_reads, length_classes):
    """sum of n_k x L_k: the bases of a mixed-length sample, an integer"""
    return sum(int(n) * int(L) for n, L in zip(class_reads, length_classes))


def read_report_classes(path):
    """The length_classes line of a report that run_pipeline wrote under mixed_lengths (`length_classes:\t<L1>\t<L2>...`), or None -
    the report has none."""
    if not os.path.isfile(path):
        raise AbundanceError("AGS report %s not found" % path)
    with open(path) as f:
        for line in f:
            if line.startswith("length_classes:"):
                txt = line.split(":", 1)[1].split()
                try:
                    return [int(x) for x in txt]
                except ValueError:
                    raise AbundanceError("AGS report %s: length_classes %r are not integers" % (path, txt))
    return None


def check_length_classes(want, valid, what):
    """A list of class lengths, sorted and without repeats; refused where one is no length the model was trained for"""
    try:
        classes = sorted(set(int(x) for x in want))
    except (TypeError, ValueError):
        raise AbundanceError("%s %r is not a list of read lengths" % (what, want))
    bad = [L for L in classes if L not in valid]
    if bad or not classes:
        raise AbundanceError("%s: length classes %s are not lengths the model was trained for: %s" % (what, bad if bad else classes, list(valid)))
    return classes


def resolve_length_classes(args, valid):
    """args['mixed_lengths'] (True or a list) to the classes of the run, or None - they are to be detected from the reads
    (microbe_census.auto_detect_length_classes): a given list; otherwise the length_classes line of args['ags_report'] where it has one.
    A list that contradicts the report's line is refused."""
    want = args["mixed_lengths"]
    given = None if want is True else check_length_classes(want, valid, "--mixed-lengths %s" % ",".join(str(x) for x in want))
    rep = read_report_classes(args["ags_report"]) if args.get("ags_report") is not None else None
    if rep is not None:
        rep = check_length_classes(rep, valid, "AGS report %s" % args["ags_report"])
        if given is not None and given != rep:
            raise AbundanceError("--mixed-lengths %s contradicts the length_classes %s of the AGS report %s: its AGS is that of other bases"
                                 % (",".join(str(x) for x in given), ",".join(str(x) for x in rep), args["ags_report"]))
    return given if given is not None else rep


def rpkg(reads, length_aa, ge):
    """reads / (gene length in kb of nucleotides: 3 x length_aa / 1000) / genome equivalents - float64, one gene or arrays."""
    return np.asarray(reads, dtype=np.float64) / (3.0 * np.asarray(length_aa, dtype=np.float64) / 1000.0) / float(ge)


def group_table(names, reads, rpkgs, group_of, detected=None):
    """[(group, genes, reads, rpkg)] in the order the groups first appear in the FASTA; a gene missing from the map is a group of its own
    name; a group's rpkg is the sum of its members' values, added in FASTA order.  With detected (0 / 1 per gene) every tuple ends with
    the group's genes_detected."""
    order, acc = [], {}
    for k, (nm, r, v) in enumerate(zip(names, reads, rpkgs)):
        g = group_of.get(nm, nm)
        if g not in acc:
            acc[g] = [0, 0, 0.0, 0]
            order.append(g)
        a = acc[g]
        a[0] += 1
        a[1] += int(r)
        a[2] += float(v)
        if detected is not None:
            a[3] += int(detected[k])
    return [(g,) + tuple(acc[g][:4 if detected is not None else 3]) for g in order]


def group_ids(names, group_of):
    """(ids, groups): every gene's group number and the groups' names, numbered in the order group_table lists them - the map that
    goes to the device (Engine.set_ties)."""
    index, ids = {}, np.zeros(len(names), np.int32)
    for k, nm in enumerate(names):
        ids[k] = index.setdefault(group_of.get(nm, nm), len(index))
    return ids, list(index)


def shared_reads(share):
    """share[] of the device (units of 2^-32) as reads: np.float64(share) / 4294967296.0"""
    return np.asarray(share, dtype=np.uint64).astype(np.float64) / SHARE_ONE


def group_ties_table(ids, ngroups, group_unique, share, rpkg_shared, detected_any=None):
    """[(unique_reads, shared_reads, rpkg_shared)] per group, in group_ids' numbering.  unique_reads is the device's group_unique - the
    reads whose whole tied set lies in the group - and NOT the sum of the members' unique_reads; shared_reads is the members' shares
    added as integers and then divided by 2^32; rpkg_shared the sum of the members' values, added in FASTA order.  With detected_any every
    tuple ends with the group's genes_detected_any."""
    acc = [[0, 0.0, 0] for _ in range(ngroups)]
    for k, g in enumerate(np.asarray(ids).tolist()):
        a = acc[g]
        a[0] += int(share[k])
        a[1] += float(rpkg_shared[k])
        if detected_any is not None:
            a[2] += int(detected_any[k])
    return [(int(group_unique[g]), float(np.float64(np.uint64(a[0])) / SHARE_ONE), a[1]) + ((a[2],) if detected_any is not None else ()) for g, a in enumerate(acc)]


def coverage_columns(length_aa, covered, spanned):
    """(breadth, mean_depth) in float64: covered_aa / length_aa and spanned / length_aa."""
    ln = np.asarray(length_aa, dtype=np.float64)
    return np.asarray(covered, dtype=np.float64) / ln, np.asarray(spanned, dtype=np.float64) / ln


def detect(reads, covered, length_aa, min_breadth):
    """1 where reads > 0 and covered_aa >= F x length_aa (covered_aa x 1 >= F x length_aa, compared in float64), otherwise 0."""
    f = np.float64(min_breadth)
    return ((np.asarray(reads) > 0) & (np.asarray(covered, dtype=np.float64) * 1 >= f * np.asarray(length_aa, dtype=np.float64))).astype(np.int64)


def depth_runs(depth, length_aa):
    """The maximal runs of equal non-zero depth, gene by gene: (gene index, start, end, depth) as arrays - start 0-based within the gene,
    end exclusive.  depth: every residue's depth, the genes one after the other (Engine.coverage_depth).  A run never crosses from one
    gene into the next, whatever the depths on either side."""
    depth = np.asarray(depth)
    length_aa = np.asarray(length_aa, dtype=np.int64)
    first = np.cumsum(length_aa) - length_aa
    if depth.size != int(length_aa.sum()):
        raise ValueError("%d depths for genes of %d residues" % (depth.size, int(length_aa.sum())))
    if depth.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    gene = np.repeat(np.arange(len(length_aa), dtype=np.int64), length_aa)
    starts = np.flatnonzero(np.r_[True, (depth[1:] != depth[:-1]) | (gene[1:] != gene[:-1])])
    ends = np.r_[starts[1:], depth.size]
    keep = depth[starts] > 0
    starts, ends = starts[keep], ends[keep]
    g = gene[starts]
    return g, starts - first[g], ends - first[g], depth[starts].astype(np.int64)


def write_depth(path, names, length_aa, depth):
    """bedGraph-style TSV of depth_runs: gene, start, end, depth - genes in FASTA order, only the genes that reads cover."""
    g, a, b, d = depth_runs(depth, length_aa)
    with open(path, "w") as out:
        out.write("#" + "\t".join(DEPTH_COLUMNS) + "\n")
        out.writelines("%s\t%d\t%d\t%d\n" % (names[k], x, y, v) for k, x, y, v in zip(g.tolist(), a.tolist(), b.tolist(), d.tolist()))


def read_depth(path, names, length_aa):
    """The public inverse of write_depth, for whoever reads the file back (a plot, a test): the depth of every residue, the genes one after
    the other as in Engine.coverage_depth() - zeros where the file has no run.  names and length_aa: the gene FASTA's, in its order."""
    length_aa = np.asarray(length_aa, dtype=np.int64)
    first = dict(zip(names, (np.cumsum(length_aa) - length_aa).tolist()))
    depth = np.zeros(int(length_aa.sum()), np.uint32)
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                continue
            nm, a, b, d = line.rstrip("\n").split("\t")
            depth[first[nm] + int(a):first[nm] + int(b)] = int(d)
    return depth


def identity_columns(idn, reads, aligned, length_aa, ge):
    """The identity columns of the gene table from Engine.identity()'s arrays: the three sums as they are; ident_mean = 100.0 x matched_aa /
    aligned_aa in float64; ident_median, ident_min, ident_max as integer percents - all four None (NA) for a gene without reads; and per level T
    reads_ident_ge<T> and rpkg_ident_ge<T>, the rpkg formula on those reads."""
    has = (np.asarray(reads) > 0) & (np.asarray(aligned) > 0)
    mean = 100.0 * np.asarray(idn["matched"], np.float64) / np.where(has, aligned, 1).astype(np.float64)
    cols = {"matched_aa": idn["matched"], "mismatched_aa": idn["mismatched"], "gap_opens": idn["gap_opens"], "ident_mean": [float(v) if h else None for v, h in zip(mean.tolist(), has.tolist())]}
    for k in ("ident_median", "ident_min", "ident_max"):
        cols[k] = [None if v < 0 else int(v) for v in np.asarray(idn[k]).tolist()]
    for j, t in enumerate(idn["levels"]):
        cols["reads_ident_ge%d" % t] = np.ascontiguousarray(idn["ge"][:, j])
        cols["rpkg_ident_ge%d" % t] = rpkg(idn["ge"][:, j], length_aa, ge)
    return cols


def tad_kept(length_aa, keep):
    """hi - lo of csrc/mc_depthstats.h: the ranks the truncated average keeps, length_aa - 2 x (length_aa x (100 - keep) // 200) - at least 1"""
    ln = np.asarray(length_aa, dtype=np.int64)
    return ln - 2 * (ln * (100 - int(keep)) // 200)


def tad(trimmed_sum, length_aa, keep):
    """the truncated average depth: trimmed_sum / (hi - lo) in float64"""
    return np.asarray(trimmed_sum, dtype=np.float64) / tad_kept(length_aa, keep).astype(np.float64)


def depth_stat_columns(ds, ds_any, length_aa, ge):
    """The depth-statistics columns of the gene table from Engine.depth_stats()'s arrays (ds; ds_any: those of the any-depth, or None):
    median_depth as it is, tad<P> = trimmed_sum / (hi - lo), tad<P>_per_ge = tad<P> / ge, and with ds_any median_depth_any and tad<P>_any."""
    P = int(ds["keep"])
    t = tad(ds["trimmed_sum"], length_aa, P)
    cols = {"median_depth": ds["median"], "tad%d" % P: t, "tad%d_per_ge" % P: t / np.float64(ge)}
    if ds_any is not None:
        cols.update({"median_depth_any": ds_any["median"], "tad%d_any" % P: tad(ds_any["trimmed_sum"], length_aa, P)})
    return cols


def depth_stat_column_kinds(table):
    """[(column, kind)] of the depth statistics, from the table's tad_keep; the _any columns only where the table has them"""
    P = table["tad_keep"]
    return [("median_depth", "d"), ("tad%d" % P, "f"), ("tad%d_per_ge" % P, "f")] + ([("median_depth_any", "d"), ("tad%d_any" % P, "f")] if table.get("median_depth_any") is not None else [])


def level_columns(levels):
    """[(column, kind)] of the levels: reads_ident_ge<T> and rpkg_ident_ge<T> per level, in the levels' order"""
    return [c for t in levels for c in (("reads_ident_ge%d" % t, "d"), ("rpkg_ident_ge%d" % t, "f"))]


def group_ident_table(names, group_of, table):
    """[(matched_aa, ident_mean, reads_ident_ge<T1>, rpkg_ident_ge<T1>, ...)] per group in group_table's order: sums over the members in FASTA
    order; ident_mean from the members' summed matched_aa and aligned_aa, None for a group without aligned residues"""
    cols = [table[name] for name, _ in level_columns(table["ident_levels"])]
    order, acc = [], {}
    for k, nm in enumerate(names):
        g = group_of.get(nm, nm)
        if g not in acc:
            acc[g] = [0, 0] + [0 if i % 2 == 0 else 0.0 for i in range(len(cols))]
            order.append(g)
        a = acc[g]
        a[0] += int(table["matched_aa"][k])
        a[1] += int(table["aligned_aa"][k])
        for i, col in enumerate(cols):
            a[2 + i] += int(col[k]) if i % 2 == 0 else float(col[k])
    return [(acc[g][0], 100.0 * acc[g][0] / acc[g][1] if acc[g][1] > 0 else None) + tuple(acc[g][2:]) for g in order]


def write_ident(path, names, hist):
    """--ident-out: gene, ident, reads - one line per non-empty bin of the histogram (Engine.identity_hist), genes in FASTA order, bins
    ascending, only the genes with reads"""
    hist = np.asarray(hist)
    g, b = np.nonzero(hist)
    with open(path, "w") as out:
        out.write("#" + "\t".join(IDENT_OUT_COLUMNS) + "\n")
        out.writelines("%s\t%d\t%d\n" % (names[k], x, v) for k, x, v in zip(g.tolist(), b.tolist(), hist[g, b].tolist()))


def read_ident(path, names):
    """The public inverse of write_ident, for whoever reads the file back (a plot, a test): uint32[genes, 101], zeros where the file has no
    line.  names: the gene FASTA's, in its order."""
    index = {nm: k for k, nm in enumerate(names)}
    hist = np.zeros((len(names), IDENT_BINS), np.uint32)
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                continue
            nm, b, v = line.rstrip("\n").split("\t")
            hist[index[nm], int(b)] = int(v)
    return hist


def ident_header_lines(table):
    return ["# identity:\ton\n"] + (["# ident_levels:\t%s\n" % ",".join(str(t) for t in table["ident_levels"])] if table["ident_levels"] else [])


def _lerp(a, b, t):
    """numpy's linear interpolation between two order statistics (numpy.percentile, method "linear"): a + (b - a) t, and from t = 0.5 on
    b - (b - a) (1 - t)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = b - a
    return np.where(t >= 0.5, b - d * (1 - t), a + d * t)


def boot_scale(ags_values, reads, read_length):
    """scale[b] = AGS_b / (L x n_b) = 1 / genome_equivalents of replicate b; NaN - the replicate is not used - where AGS_b is None or
    the replicate drew no read"""
    return np.array([float("nan") if a is None or n <= 0 else float(a) / (float(read_length) * float(n)) for a, n in zip(ags_values, reads)], np.float64)


def boot_columns(stats, used, length_aa):
    """(rpkg_boot_se, rpkg_ci95_low, rpkg_ci95_high) from the device's six doubles per gene (csrc/mc_geneboot.h: sum, m2 and the order
    statistics x[lo], x[lo + 1], x[hi], x[hi + 1] of the `used` replicate values reads_b / genome_equivalents_b) - with
    kb = 3 x length_aa / 1000: se = sqrt(m2 / (used - 1)) / kb, NaN with used < 2; the interval is numpy.percentile(values / kb,
    [2.5, 97.5]): the order statistics divided by kb, interpolated at the fraction of (used - 1) x 0.025 and (used - 1) x 0.975."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 6)
    kb = 3.0 * np.asarray(length_aa, dtype=np.float64) / 1000.0
    m = int(used)
    if m < 1:
        nan = np.full(len(kb), np.nan)
        return nan, nan.copy(), nan.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(stats[:, 1] / (m - 1)) / kb if m > 1 else np.full(len(kb), np.nan)
        out = []
        for q, col in ((0.025, 2), (0.975, 4)):
            v = (m - 1) * q
            out.append(_lerp(stats[:, col] / kb, stats[:, col + 1] / kb, v - math.floor(v)))
    return se, out[0], out[1]


def group_boot_columns(stats, used):
    """(rpkg_boot_se, rpkg_ci95_low, rpkg_ci95_high) of the groups from the device's six doubles per group (csrc/mc_groupboot.h: sum, m2 and
    the order statistics of the `used` replicate values, every one a sum of the members' replicate RPKGs): se = sqrt(m2 / (used - 1)), NaN with
    used < 2; the interval is numpy.percentile(values, [2.5, 97.5]) by boot_columns' interpolation.  No division by a length: it is inside
    the values."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 6)
    m = int(used)
    if m < 1:
        nan = np.full(len(stats), np.nan)
        return nan, nan.copy(), nan.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(stats[:, 1] / (m - 1)) if m > 1 else np.full(len(stats), np.nan)
        out = []
        for q, col in ((0.025, 2), (0.975, 4)):
            v = (m - 1) * q
            out.append(_lerp(stats[:, col], stats[:, col + 1], v - math.floor(v)))
    return se, out[0], out[1]


def coverage_need(length_aa, min_breadth):
    """need[g] = max(1, ceil(F x length_aa)) in float64, as uint32: the integer form of detect()'s comparison - an integer covered_aa is
    >= F x length_aa exactly when it is >= ceil(F x length_aa), and need >= 1 makes reads > 0 implied (csrc/mc_covboot.h, DETECTION)"""
    return np.maximum(1.0, np.ceil(np.float64(min_breadth) * np.asarray(length_aa, dtype=np.float64))).astype(np.uint32)


def cov_boot_columns(stats, B, length_aa):
    """(breadth_boot_mean, breadth_boot_se, breadth_ci95_low, breadth_ci95_high) from the device's six doubles per gene (csrc/mc_covboot.h: sum,
    m2 and the order statistics x[lo], x[lo + 1], x[hi], x[hi + 1] of the B replicate values covered_b, in residues): mean = sum / B /
    length_aa, se = sqrt(m2 / (B - 1)) / length_aa, NaN with B < 2; the interval is numpy.percentile(covered_b / length_aa, [2.5, 97.5]) by
    boot_columns' interpolation."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 6)
    ln = np.asarray(length_aa, dtype=np.float64)
    m = int(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = stats[:, 0] / m / ln
        se = np.sqrt(stats[:, 1] / (m - 1)) / ln if m > 1 else np.full(len(ln), np.nan)
        out = []
        for q, col in ((0.025, 2), (0.975, 4)):
            v = (m - 1) * q
            out.append(_lerp(stats[:, col] / ln, stats[:, col + 1] / ln, v - math.floor(v)))
    return mean, se, out[0], out[1]


def header_lines(args, table):
    mixed = [] if table.get("length_classes") is None else [(k, ",".join(str(int(x)) for x in table[k])) for k in ("length_classes", "class_reads", "class_reads_assigned")] + [("sampled_bases", table["sampled_bases"])]
    h = [("metagenome", ",".join(args["seqfiles"])), ("genes", args["genes"]), ("sampled_reads", table["sampled_reads"]),
         ("trimmed_length", table["trimmed_length"])] + mixed + [("min_ident", args["min_ident"]), ("min_aln", args["min_aln"]), ("min_bits", repr(float(args["min_bits"]))),
         ("average_genome_size", repr(float(table["ags"]))), ("ags_source", table["ags_source"]),
         ("genome_equivalents_sampled", repr(float(table["genome_equivalents_sampled"]))), ("reads_assigned", table["reads_assigned"])]
    if table.get("covered_aa") is not None:
        h.append(("coverage", "on"))
    if table.get("detected") is not None:
        h += [("min_breadth", repr(float(table["min_breadth"]))), ("genes_detected", int(np.sum(table["detected"])))]
    if table.get("unique_reads") is not None:
        h += [("ties", "on"), ("reads_ambiguous", table["reads_ambiguous"])]
        if table.get("reads_ambiguous_across_groups") is not None:
            h.append(("reads_ambiguous_across_groups", table["reads_ambiguous_across_groups"]))
    if table.get("curve") is not None:
        h.append(("curve", len(table["curve"]["points"])))
    if table.get("long_genes") is not None:
        h += [("long_genes", "on")] + [(k, table["long_genes"][k]) for k in ("genes_split", "segments", "edge_rows")]
    return ["# %s:\t%s\n" % kv for kv in h]


def table_columns(table):
    """[(column, kind)] of the gene table, from the keys the table has - kind s: the value as it is, d: %d, f: repr(float()), n: f or NA"""
    has = lambda key: table.get(key) is not None
    groups = ((True, COLUMNS, "sdddf"), (has("covered_aa"), COVERAGE_COLUMNS, "dffd"), (has("detected"), ("detected",), "d"), (has("unique_reads"), TIES_COLUMNS, "ddff"),
              (has("covered_any_aa"), TIES_COVERAGE_COLUMNS, "df"), (has("detected_any"), ("detected_any",), "d"), (has("rpkg_boot_se"), BOOT_COLUMNS, "fff"),
              (has("rpkg_shared_boot_se"), TIE_BOOT_COLUMNS, "fff"), (has("breadth_boot_se"), COV_BOOT_COLUMNS, "ffff"), (has("detected_support"), ("detected_support",), "f"),
              (has("identity"), IDENT_COLUMNS, "dddniii"))
    return ([c for on, names, kinds in groups if on for c in zip(names, kinds)] + (level_columns(table["ident_levels"]) if has("identity") else []) +
            (depth_stat_column_kinds(table) if has("depth_stats") else []))


def group_columns(table):
    """[(column, kind)] of the groups table: those of a row of table['groups'] and, with ties, of the same row of table['groups_ties']"""
    gt = table.get("groups_ties")
    ties = GROUP_TIES_COLUMNS + (("genes_detected_any",) if table.get("detected_any") is not None else ()) if gt is not None else ()
    boot = BOOT_COLUMNS if table.get("groups_boot") is not None else ()
    ident = [("matched_aa", "d"), ("ident_mean", "n")] + level_columns(table["ident_levels"]) if table.get("groups_ident") is not None else []
    return list(zip(GROUP_COLUMNS + (("genes_detected",) if table.get("detected") is not None else ()), "sddfd")) + list(zip(ties, "dffd")) + list(zip(boot, "fff")) + ident


def _write_rows(out, columns, values):
    """the header line and the rows of a table, both from ONE list of (column, kind); values: the columns' values, a sequence per column"""
    out.write("\t".join(name for name, _ in columns) + "\n")
    text = [[TEXT[kind](v) for v in (col.tolist() if isinstance(col, np.ndarray) else col)] for (_, kind), col in zip(columns, values)]
    out.writelines("\t".join(row) + "\n" for row in zip(*text))


def boot_header_lines(table):
    """the four header lines of a bootstrapped table"""
    return ["# %s:\t%s\n" % kv for kv in (("bootstrap", table["bootstrap"]), ("bootstrap_seed", table["bootstrap_seed"]),
                                          ("bootstrap_replicates", "%d/%d" % (table["boot_used"], table["bootstrap"])),
                                          ("bootstrap_denominator", table["bootstrap_denominator"]))]


def write_table(path, args, table):
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        if table.get("rpkg_boot_se") is not None:
            out.writelines(boot_header_lines(table))
        if table.get("rpkg_shared_boot_se") is not None:
            out.writelines(["# bootstrap_ties:\ton\n", "# tie_list:\t%d/%d\n" % (table["tie_list_entries"], table["tie_list_capacity"])])
        if table.get("breadth_boot_se") is not None:
            out.write("# bootstrap_coverage:\ton\n")
        if table.get("identity") is not None:
            out.writelines(ident_header_lines(table))
        if table.get("depth_stats") is not None:
            out.writelines(["# depth_stats:\ton\n", "# tad_keep:\t%d\n" % table["tad_keep"]])
        columns = table_columns(table)
        _write_rows(out, columns, [table[name] for name, _ in columns])


def write_groups(path, args, table):
    """the groups table; it bootstraps only with table['groups_boot'] (bootstrap_groups): without it the file is what it was before the switch existed"""
    boot = table.get("groups_boot")
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        out.write("# groups:\t%s\n" % args["groups"])
        if boot is not None:
            out.writelines(boot_header_lines(table) + ["# bootstrap_groups:\ton\n"])
        if table.get("groups_ident") is not None:
            out.writelines(ident_header_lines(table))
        _write_rows(out, group_columns(table), list(zip(*table["groups"])) + list(zip(*(table.get("groups_ties") or []))) + list(zip(*(boot or []))) + list(zip(*(table.get("groups_ident") or []))))


def curve_figures(names, length_aa, read_length, points, reads, aligned, covered, ags, min_breadth=None, group_of=None):
    """table['curve'] from the device's arrays: points n_k, reads / aligned / covered (or None) as [K, genes], ags: one value per point
    (None: no estimate at that point - its AGS, genome equivalents and RPKG are None / NaN).  Every figure comes from the lines the
    gene table is made with: genome_equivalents, rpkg, detect, group_table."""
    K = len(points)
    cu = {"points": [int(n) for n in points], "reads": reads, "aligned_aa": aligned, "ags": [None if a is None else float(a) for a in ags],
          "genome_equivalents_sampled": [], "rpkg": np.full((K, len(names)), np.nan), "reads_assigned": [int(x) for x in reads.sum(axis=1)],
          "genes_with_reads": [int(x) for x in (reads > 0).sum(axis=1)]}
    for k, n_k in enumerate(cu["points"]):
        ge = None if cu["ags"][k] is None else genome_equivalents(n_k, read_length, cu["ags"][k])
        cu["genome_equivalents_sampled"].append(ge)
        if ge is not None:
            cu["rpkg"][k] = rpkg(reads[k], length_aa, ge)
    if covered is not None:
        cu["covered_aa"] = covered
        if min_breadth is not None:
            cu["detected"] = np.stack([detect(reads[k], covered[k], length_aa, min_breadth) for k in range(K)])
            cu["genes_detected"] = [int(x) for x in cu["detected"].sum(axis=1)]
    if group_of is not None:
        cu["groups"] = [group_table(names, reads[k], cu["rpkg"][k], group_of, cu["detected"][k] if "detected" in cu else None) for k in range(K)]
        cu["groups_with_reads"] = [sum(1 for g in gt if g[2] > 0) for gt in cu["groups"]]
    return cu


def write_curve(path, args, table):
    """<outfile>.curve.tsv: the gene table's header lines, then one row per point"""
    cu = table["curve"]
    more = tuple(k for k in ("genes_detected", "groups_with_reads") if k in cu)
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        _write_rows(out, list(zip(CURVE_COLUMNS + more, "dnndddd")),
                    [cu[k] for k in ("points", "ags", "genome_equivalents_sampled", "reads_assigned", "genes_with_reads") + more])


def write_curve_genes(path, table):
    """--curve-genes: gene, reads_1 .. reads_K and with coverage covered_aa_1 .. covered_aa_K - genes in FASTA order"""
    cu = table["curve"]
    mats = [("reads", cu["reads"])] + ([("covered_aa", cu["covered_aa"])] if cu.get("covered_aa") is not None else [])
    with open(path, "w") as out:
        out.write("# curve_points:\t%s\n" % "\t".join(str(n) for n in cu["points"]))
        _write_rows(out, [("gene", "s")] + [("%s_%d" % (what, k + 1), "d") for what, m in mats for k in range(len(m))],
                    [table["gene"]] + [at_k for _, m in mats for at_k in m])


def read_table(path):
    """(header dict of strings, rows as lists of strings) of a table write_table / write_groups wrote."""
    header, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("# "):
                k, v = line[2:].rstrip("\n").split(":\t", 1)
                header[k] = v
            else:
                rows.append(line.rstrip("\n").split("\t"))
    return header, rows[1:]


def _pipeline_args(args):
    # (nreads None is run_pipeline's "no cap" and is handed on; any other key that is None is left to impute_missing_args)
    return {k: (list(args[k]) if k == "seqfiles" else args[k]) for k in PIPELINE_KEYS if k in args and (args[k] is not None or k == "nreads")}


def _check_int(args, key, lo, hi, span):
    """args[key] becomes an int; refused where it is none (a bool is none) or lies outside lo .. hi"""
    v = args[key]
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise AbundanceError("--%s %s is not an integer from %s" % (key.replace("_", "-"), v, span))
    args[key] = int(v)


def _check_switch(args, key):
    if not isinstance(args[key], (bool, int)) or args[key] not in (0, 1):
        raise AbundanceError("%s %r is not a switch: True or False" % (key, args[key]))
    args[key] = bool(args[key])


def _check_own_path(args, key, others):
    """refused: args[key] is the path of another file of the run - of <outfile> + a suffix (the groups table only with groups, the curve table only
    with curve when it is asked about by name) or of --depth-out / --curve-genes"""
    what = {"": "the gene table itself", ".curve.tsv": "the curve table (<outfile>.curve.tsv)", ".groups.tsv": "the groups table (<outfile>.groups.tsv)",
            "depth_out": "the depth file (--depth-out)", "curve_genes": "the curve's per-gene matrix (--curve-genes)"}
    for o in others:
        other = args[o] if o in ("depth_out", "curve_genes") else args["outfile"] + o if args.get("outfile") and (o != ".groups.tsv" or args["groups"]) and (o != ".curve.tsv" or args["curve"] is not None) else None
        if other and os.path.abspath(args[key]) == os.path.abspath(other):
            raise AbundanceError("--%s %s is the path of %s: two files" % (key.replace("_", "-"), args[key], what[o]))


def check_request(args):
    """Everything that can be refused before any GPU work; returns (names, seqs, group_of, ags or None, ags_source or None)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.get("distributed"):
        raise AbundanceError("Gene abundances are not computed by a distributed run (WORLD_SIZE %s): run one process" % os.environ.get("WORLD_SIZE", "1"))
    for key, default in (("min_ident", 0), ("min_aln", 0), ("min_bits", 0.0), ("groups", None), ("ags", None), ("ags_report", None),
                         ("coverage", False), ("min_breadth", None), ("depth_out", None), ("ties", False), ("curve", None), ("curve_genes", None),
                         ("bootstrap", None), ("bootstrap_seed", None), ("bootstrap_groups", False), ("mixed_lengths", None), ("long_genes", False),
                         ("bootstrap_ties", False), ("tie_list_factor", None), ("bootstrap_coverage", False), ("identity", False), ("ident_levels", None), ("ident_out", None),
                         ("depth_stats", False), ("tad_keep", None)):
        args.setdefault(key, default)
    mixed = microbe_census.mixed_lengths_on(args)
    if mixed:
        ml = "" if args["mixed_lengths"] is True else " %s" % ",".join(str(x) for x in args["mixed_lengths"])
        if args.get("read_length") is not None:
            raise AbundanceError("--mixed-lengths%s cannot be combined with -l %s: every read is cut to its own length class" % (ml, args["read_length"]))
        if args["curve"] is not None:
            raise AbundanceError("--mixed-lengths%s cannot be combined with --curve %s: rarefying reads of mixed lengths needs the bases of every prefix" % (ml, args["curve"]))
        if args["bootstrap"] is not None and args["ags"] is None and args["ags_report"] is None:
            raise AbundanceError("--mixed-lengths%s with --bootstrap %s needs --ags or --ags-report: the default AGS is run_pipeline's, which does not bootstrap "
                                 "an estimate of mixed lengths" % (ml, args["bootstrap"]))
    if args["curve"] is not None:
        _check_int(args, "curve", 1, MAX_CURVE, "1 to %d" % MAX_CURVE)
    if args["bootstrap"] is not None:
        _check_int(args, "bootstrap", 1, MAX_BOOT, "1 to %d" % MAX_BOOT)
        if args["curve"] is not None:
            raise AbundanceError("--bootstrap %d cannot be combined with --curve %d: the curve's points are not bootstrapped" % (args["bootstrap"], args["curve"]))
    if args["bootstrap_seed"] is not None:
        if args["bootstrap"] is None:
            raise AbundanceError("--bootstrap-seed %s needs --bootstrap B: it seeds the replicates" % (args["bootstrap_seed"],))
        _check_int(args, "bootstrap_seed", 0, (1 << 64) - 1, "0 to 2^64 - 1")
    _check_switch(args, "bootstrap_groups")
    if args["bootstrap_groups"]:
        if args["bootstrap"] is None:
            raise AbundanceError("--bootstrap-groups needs --bootstrap B (--bootstrap %s): it sums the gene bootstrap's replicates over every group" % (args["bootstrap"],))
        if not args["groups"]:
            raise AbundanceError("--bootstrap-groups needs --groups map.tsv (--groups %s): it bootstraps the groups table" % (args["groups"],))
    if args["curve_genes"] is not None:
        if not args["curve_genes"]:
            raise AbundanceError("--curve-genes %r is an empty path" % (args["curve_genes"],))
        if args["curve"] is None:
            raise AbundanceError("--curve-genes %s needs --curve K: it writes the curve's per-gene matrix" % (args["curve_genes"],))
        _check_own_path(args, "curve_genes", ("", ".curve.tsv", ".groups.tsv", "depth_out"))
    if args["min_breadth"] is not None:
        f = args["min_breadth"]
        try:
            f = float("nan") if isinstance(f, bool) else float(f)
        except (TypeError, ValueError):
            f = float("nan")
        if not 0.0 < f <= 1.0:                                   # (NaN compares false)
            raise AbundanceError("--min-breadth %s is not a fraction in (0, 1]" % (args["min_breadth"],))
        args["min_breadth"] = f
    if args["depth_out"] is not None:
        if not args["depth_out"]:
            raise AbundanceError("--depth-out %r is an empty path" % (args["depth_out"],))
        _check_own_path(args, "depth_out", ("", ".groups.tsv"))
    _check_switch(args, "ties")
    _check_switch(args, "bootstrap_ties")
    if args["bootstrap_ties"]:
        if args["bootstrap"] is None:
            raise AbundanceError("--bootstrap-ties needs --bootstrap B (--bootstrap %s): it sums the gene bootstrap's weights over every gene's tied reads" % (args["bootstrap"],))
        if not args["ties"]:
            raise AbundanceError("--bootstrap-ties needs --ties (--ties %s): it bootstraps rpkg_shared" % (args["ties"],))
    if args["tie_list_factor"] is not None:
        if not args["bootstrap_ties"]:
            raise AbundanceError("--tie-list-factor %s needs --bootstrap-ties: it sizes the list of tie entries" % (args["tie_list_factor"],))
        _check_int(args, "tie_list_factor", 1, MAX_TIE_FACTOR, "1 to %d" % MAX_TIE_FACTOR)
    _check_switch(args, "depth_stats")
    if args["tad_keep"] is not None:
        _check_int(args, "tad_keep", 1, 100, "1 to 100")
    args["depth_stats"] = args["depth_stats"] or args["tad_keep"] is not None
    if args["depth_stats"] and args["tad_keep"] is None:
        args["tad_keep"] = TAD_KEEP
    args["coverage"] = bool(args["coverage"]) or args["min_breadth"] is not None or args["depth_out"] is not None or args["depth_stats"]
    _check_switch(args, "bootstrap_coverage")
    if args["bootstrap_coverage"]:
        if args["bootstrap"] is None:
            raise AbundanceError("--bootstrap-coverage needs --bootstrap B (--bootstrap %s): it covers every gene with the reads of the gene bootstrap's replicates" % (args["bootstrap"],))
        if not args["coverage"]:
            raise AbundanceError("--bootstrap-coverage needs --coverage, --min-breadth or --depth-out (--coverage %s): it bootstraps breadth and detected" % (args["coverage"],))
    _check_switch(args, "identity")
    if args["ident_levels"] is not None:
        lv = args["ident_levels"]
        ok = isinstance(lv, (list, tuple)) and 1 <= len(lv) <= MAX_IDENT_LEVELS and all(not isinstance(t, bool) and isinstance(t, (int, np.integer)) and 0 <= int(t) <= 100 for t in lv)
        if not ok or any(int(b) <= int(a) for a, b in zip(lv, lv[1:])):
            raise AbundanceError("--ident-levels %s is not a list of 1 to %d integer percents from 0 to 100, strictly ascending"
                                 % (",".join(str(t) for t in lv) if isinstance(lv, (list, tuple)) else lv, MAX_IDENT_LEVELS))
        args["ident_levels"] = [int(t) for t in lv]
    if args["ident_out"] is not None:
        if not args["ident_out"]:
            raise AbundanceError("--ident-out %r is an empty path" % (args["ident_out"],))
        _check_own_path(args, "ident_out", ("", ".curve.tsv", ".groups.tsv", "depth_out", "curve_genes"))
    args["identity"] = args["identity"] or args["ident_levels"] is not None or args["ident_out"] is not None
    if args["ags"] is not None and args["ags_report"] is not None:
        raise AbundanceError("--ags %s and --ags-report %s cannot be combined: one AGS" % (args["ags"], args["ags_report"]))
    mi = args["min_ident"]
    if isinstance(mi, bool) or mi != int(mi) or not 0 <= int(mi) <= 100:
        raise AbundanceError("--min-ident %s is not an integer percent from 0 to 100" % (mi,))
    if isinstance(args["min_aln"], bool) or args["min_aln"] != int(args["min_aln"]) or int(args["min_aln"]) < 0:
        raise AbundanceError("--min-aln %s is not a non-negative integer" % (args["min_aln"],))
    if math.isnan(float(args["min_bits"])):
        raise AbundanceError("--min-bits %s is not a number" % (args["min_bits"],))
    args["min_ident"], args["min_aln"], args["min_bits"] = int(mi), int(args["min_aln"]), float(args["min_bits"])
    ags, source = (check_ags(args["ags"], "--ags"), "--ags") if args["ags"] is not None else (None, None)
    _check_switch(args, "long_genes")
    names, seqs = read_genes(args["genes"], args["long_genes"])
    args["gene_fold"] = split_genes(names, seqs) if args["long_genes"] else None      # (refused here: before any GPU work)
    group_of = read_groups(args["groups"], names) if args["groups"] else None
    if args["ags_report"] is not None:
        source = "report %s" % args["ags_report"]
        ags = check_ags(read_ags_report(args["ags_report"]), source)
    if mixed:                   # (None: to be detected from the reads, once the files are known to be there)
        args["length_classes"] = resolve_length_classes(args, list(microbe_census._valid_read_lengths(args.get("model_dir"))))
    return names, seqs, group_of, ags, source


def resolve_sample(args, ags, source):
    """Stage 1 - the record `sample`: ags and source (given, or run_pipeline's estimate on the same files under the same options), pargs (its
    args - of that run, or of the imputation it makes, without a search), classes (of mixed_lengths, else None), L (the trimmed length or "mixed")"""
    mixed, classes = microbe_census.mixed_lengths_on(args), None
    if mixed:                   # neither a list nor a report's line: the classes run_pipeline would detect on the same file
        classes = args["length_classes"]
        if classes is None:
            try:
                classes = microbe_census.auto_detect_length_classes(args["seqfiles"][0], list(microbe_census._valid_read_lengths(args.get("model_dir"))))
            except SystemExit as e:
                raise AbundanceError(str(e))
        args["length_classes"] = classes = [int(x) for x in classes]
    if ags is None:
        more = {"curve": args["curve"]} if args["curve"] else {"bootstrap": args["bootstrap"], "bootstrap_seed": args["bootstrap_seed"] or 0} if args["bootstrap"] else {}
        more = {"mixed_lengths": list(classes)} if mixed else more       # (check_request has refused the curve and the bootstrap of a default AGS)
        est = microbe_census.run_pipeline(dict(_pipeline_args(args), **more) if more else _pipeline_args(args))
        if est is None:
            raise AbundanceError("run_pipeline gave no AGS estimate for %s" % ",".join(args["seqfiles"]))
        source = "run_pipeline"
        ags, pargs = check_ags(est[0], source), est[1]
    else:                       # the same imputation run_pipeline makes (file type, quality offset, read length)
        pargs = _pipeline_args(args)
        microbe_census._cap_host_threads(pargs.get("threads"))
        if mixed:               # (as run_pipeline: read_length becomes "mixed" and is not detected)
            pargs["mixed_lengths"] = list(classes)
            microbe_census.check_mixed_lengths(pargs)
        microbe_census.impute_missing_args(pargs)
        microbe_census.check_arguments(pargs)
    return {"ags": ags, "source": source, "pargs": pargs, "classes": classes, "L": "mixed" if mixed else int(pargs["read_length"])}


def _set_switches(eng, args, sample, names, group_of):
    """fold, run or run_classes, abundance, coverage, ties, identity, abundance_classes; returns (gids, gnames): the groups the device got, or None twice"""
    fold, classes = args["gene_fold"], sample["classes"]
    if fold is not None:        # long_genes: the engine is open on the segments, every counter is in gene space
        eng.set_gene_fold(fold["seg_gene"], fold["seg_off"], fold["gene_len"])
    if classes is not None:     # (the default parameters: classification does not enter the counts)
        eng.set_run_classes(classes)
    else:
        eng.set_run(sample["L"])
    eng.set_abundance(True, min_ident=args["min_ident"], min_aln=args["min_aln"], min_bits=args["min_bits"])
    if args["coverage"]:
        eng.set_coverage(True)
    gids, gnames = group_ids(names, group_of) if args["ties"] and group_of is not None else (None, None)
    if args["ties"]:
        eng.set_ties(True, gids, len(gnames or ()))
    if args.get("identity"):
        eng.set_identity(True)
    if classes is not None:
        eng.set_abundance_classes(True)
    return gids, gnames


def tie_list_capacity(gene_capacity, factor):
    """the entries of the tie list: min(2^27, factor x the gene list's capacity), factor None: the default"""
    return min(MAX_TIE_LIST, int(TIE_FACTOR if factor is None else factor) * int(gene_capacity))


def tie_list_overflow(dropped, candidates_sum, gene_capacity, factor):
    """the refusal of a run whose tied sets did not fit the tie list: the entries dropped and the smallest factor that would have fitted,
    ceil(sum(candidates) / the gene list's capacity)"""
    fits = -(-int(candidates_sum) // max(int(gene_capacity), 1))
    return AbundanceError("--bootstrap-ties: %d tie entries did not fit the list of %d (--tie-list-factor %d x %d reads): --tie-list-factor %d fits all %d"
                          % (dropped, tie_list_capacity(gene_capacity, factor), TIE_FACTOR if factor is None else factor, gene_capacity, fits, candidates_sum))


def _size_lists(eng, args, n):
    """the gene bootstrap's list of n reads and, with bootstrap_ties, the tie list behind it, with bootstrap_coverage the coverage list: one moment, one count"""
    eng.set_gene_bootstrap(n)
    if args["bootstrap_ties"] and n:
        eng.set_tie_bootstrap(tie_list_capacity(n, args["tie_list_factor"]))
    if args["bootstrap_coverage"] and n:                            # (one entry per assigned read: no more than the reads)
        eng.set_coverage_bootstrap(n)


def _search_once(eng, rd, args, sample):
    """The one search of a run - no m8 row reaches the host; returns (cu, points): Engine.curve() and the curve's points, or None twice.
    The bootstrap's list of read ids is sized before the search: by -n, the sampler sampling beside the search, or - no cap - by the reads the
    sampler takes; the curve's points depend on that number too: there it runs to its end first, and no read taken means no search."""
    B, cap = args["bootstrap"], sample["pargs"]["nreads"]
    if B and cap is not None:
        _size_lists(eng, args, int(cap))
    if not args["curve"] and not (B and cap is None):
        eng.search_files(rd, keep_rows=False)
        return None, None
    n = rd.run()
    if not n:
        return None, None
    points = microbe_census.curve_points(n, args["curve"]) if args["curve"] else None
    if points is None:
        _size_lists(eng, args, n)
    else:
        eng.set_curve(points)
    (eng.search if sample["classes"] is None else eng.search_classes)(rd.reads(n), keep_rows=False)
    return (None, None) if points is None else (eng.curve(covered=bool(args["coverage"])), points)


def _replicate_scale(args, sample, ab, ac):
    """scale[b] = 1 / the genome equivalents of replicate b: run_pipeline's replicates under its AGS, B times the sample's under a given one"""
    B, pargs = args["bootstrap"], sample["pargs"]
    if sample["source"] == "run_pipeline":
        if len(pargs.get("ags_boot_values") or []) != B or len(pargs.get("ags_boot_reads") or []) != B:
            raise AbundanceError("run_pipeline gave %d replicate AGS values for --bootstrap %d" % (len(pargs.get("ags_boot_values") or []), B))
        return boot_scale(pargs["ags_boot_values"], pargs["ags_boot_reads"], sample["L"])
    return np.full(B, 1.0 / (sampled_bases(ac["rows"], sample["classes"]) / sample["ags"] if ac is not None else genome_equivalents(ab["searched"], sample["L"], sample["ags"])))


def device_pass(args, sample, names, seqs, group_of):
    """Stage 2 - the record `counts`, from the only place that opens a reader or an engine: what the device counted as numpy arrays and ints - ab,
    ac, cov, depth, ti, tcov, cu and points, gb, gbg (the groups') and scale, idn (the identity's figures, with the histogram under "hist" for ident_out), ds and ds_any (the depth statistics), fold_stats (None: not asked for), sampled, gids and gnames, search_ms and the *_ms"""
    pargs, classes, fold = sample["pargs"], sample["classes"], args["gene_fold"]
    sampler = (pargs["nreads"], pargs["file_type"] == "fastq", pargs.get("quality_offset") or 0, pargs["min_quality"], pargs["mean_quality"], pargs["max_unknown"], pargs["filter_dups"])
    rd = _native.Reader.with_classes(pargs["seqfiles"], classes, *sampler) if classes is not None else _native.Reader(pargs["seqfiles"], sample["L"], *sampler)
    eng = None
    try:                        # (long_genes: the engine on the segments, with the genes' statistics)
        db = {"names": names, "seqs": seqs} if fold is None else {"names": fold["seg_names"], "seqs": fold["seg_seqs"], "stats": fold["stats"]}
        eng = _native.Engine(device=int(args.get("device") or 0), marker_family=[0] * len(db["names"]), nfam=1, **db)
        c = dict.fromkeys(("ac", "gb", "gbg", "scale", "tb", "cb", "idn", "ds", "ds_any"))
        c["gids"], c["gnames"] = _set_switches(eng, args, sample, names, group_of)
        try:
            c["cu"], c["points"] = _search_once(eng, rd, args, sample)
        except _native.ReferenceError_ as e:
            raise AbundanceError(str(e))
        c["ab"] = eng.abundance()
        if classes is not None:
            c["ac"], c["abundance_classes_ms"] = eng.abundance_classes(), eng.abundance_classes_ms()
        if args["bootstrap"] and c["ab"]["searched"]:
            c["scale"] = _replicate_scale(args, sample, c["ab"], c["ac"])
            try:
                c["gb"] = eng.gene_bootstrap(args["bootstrap"], args["bootstrap_seed"] or 0, c["scale"])
            except RuntimeError as e:
                raise AbundanceError(str(e))
            c["gene_bootstrap_ms"] = eng.gene_bootstrap_ms()
            if args["bootstrap_groups"]:                            # the same replicates and scales, summed over group_ids' groups on the device
                ids, gn = group_ids(names, group_of)
                try:
                    c["gbg"] = eng.group_bootstrap(args["bootstrap"], args["bootstrap_seed"] or 0, c["scale"], ids, len(gn), 3.0 * np.array([len(s) for s in seqs], np.float64) / 1000.0)
                except RuntimeError as e:
                    raise AbundanceError(str(e))
                c["group_bootstrap_ms"] = eng.group_bootstrap_ms()
            if args["bootstrap_ties"]:                              # the same replicates and scales on the shares of every tied set
                glist = eng.gene_bootstrap_capacity
                total, cap_t = int(eng.ties()["candidates"].sum()), tie_list_capacity(glist, args["tie_list_factor"])      # (the tie table knows the sum whether or not the list held it)
                try:
                    c["tb"] = eng.tie_bootstrap(args["bootstrap"], args["bootstrap_seed"] or 0, c["scale"])
                except RuntimeError as e:
                    raise tie_list_overflow(total - cap_t, total, glist, args["tie_list_factor"]) if total > cap_t else AbundanceError(str(e))
                c["tie_list"] = (total, cap_t)
                c["tie_bootstrap_ms"] = eng.tie_bootstrap_ms()
            if args["bootstrap_coverage"]:                          # the same replicates: what the reads present in each of them cover
                need = coverage_need([len(s) for s in seqs], args["min_breadth"]) if args["min_breadth"] is not None else None
                try:
                    c["cb"] = eng.coverage_bootstrap(args["bootstrap"], args["bootstrap_seed"] or 0, need)
                except RuntimeError as e:
                    raise AbundanceError(str(e))
                c["coverage_bootstrap_ms"] = eng.coverage_bootstrap_ms()
        c["cov"] = eng.coverage() if args["coverage"] else None
        c["depth"] = eng.coverage_depth() if args["depth_out"] is not None else None
        c["ti"] = eng.ties() if args["ties"] else None
        c["tcov"] = eng.ties_coverage() if args["ties"] and args["coverage"] else None
        if args.get("depth_stats"):                                 # the selection runs on the device: four integers per gene come over, no depth
            c["ds"] = eng.depth_stats(args["tad_keep"])
            c["ds_any"] = eng.depth_stats(args["tad_keep"], any=True) if args["ties"] else None
            c["depth_stats_ms"] = eng.depth_stats_ms()
        if args.get("identity"):                                    # the scan runs on the device; the histogram itself comes over only for ident_out
            c["idn"] = eng.identity(args["ident_levels"] or ())
            if args["ident_out"] is not None:
                c["idn"]["hist"] = eng.identity_hist()
            c["identity_ms"] = eng.identity_ms()
        c["fold_stats"] = eng.gene_fold_stats() if fold is not None else None
        c["abundance_ms"], c["search_ms"] = eng.abundance_ms(), eng.stats()["ms_total"]
        if args["coverage"]:
            c["coverage_ms"] = eng.coverage_ms()
        if args["ties"]:
            c["ties_ms"] = eng.ties_ms()
        if c["cu"] is not None:
            c["curve_ms"] = eng.curve_ms()
        c["sampled"] = int(rd.stats()["sampled"])
    finally:
        rd.close()
        if eng is not None:
            eng.close()
    return c


def build_table(args, sample, counts, names, seqs, group_of):
    """Stage 3 - the table from the two records, in numpy and Python alone (no engine, no reader, no file): the refusals that compare them,
    every column, groups, curve and long_genes - and what the run leaves in args"""
    ags, source, pargs, classes, L = (sample[k] for k in ("ags", "source", "pargs", "classes", "L"))
    ab, ac, cov, ti, tcov, cu, gb, fs = (counts[k] for k in ("ab", "ac", "cov", "ti", "tcov", "cu", "gb", "fold_stats"))
    mixed, sampled, est = classes is not None, counts["sampled"], source == "run_pipeline"
    if sampled == 0:
        raise AbundanceError("No reads remaining after filtering")
    if "sampled_reads" in pargs and int(pargs["sampled_reads"]) != sampled or ab["searched"] != sampled:
        raise AbundanceError("the gene search saw %d reads (%d sampled), the AGS estimate %s" % (ab["searched"], sampled, pargs.get("sampled_reads")))
    class_reads = class_assigned = None
    if mixed:
        K = len(classes)
        class_reads, class_assigned = [int(x) for x in ac["rows"][:K]], [int(x) for x in ac["assigned"][:K]]
        if sum(class_reads) != sampled or int(ac["rows"][K]) != 0 or est and (list(pargs.get("length_classes") or []) != classes or list(pargs.get("class_reads") or []) != class_reads):
            raise AbundanceError("the gene search saw %d reads (%d sampled): %s reads in the classes %s and %d below them, the AGS estimate %s in the classes %s"
                                 % (ab["searched"], sampled, class_reads, classes, int(ac["rows"][K]), pargs.get("class_reads") if est else "-", pargs.get("length_classes") if est else "-"))
        args["class_reads"] = class_reads
    args.update((k, pargs[k]) for k in ("file_type", "quality_offset", "read_length", "nreads", "min_quality", "mean_quality", "filter_dups", "max_unknown") + (
        ("ags_boot_se", "ags_ci95", "ags_boot_replicates", "ags_boot_values", "ags_boot_reads") if gb is not None and est else ()) if k in pargs)
    args["sampled_reads"] = sampled
    args.update((k, v) for k, v in counts.items() if k.endswith("_ms"))
    length_aa = np.array([len(s) for s in seqs], np.int64)
    bases = sampled_bases(class_reads, classes) if mixed else None
    ge = bases / ags if mixed else genome_equivalents(sampled, L, ags)
    table = {"gene": list(names), "length_aa": length_aa, "reads": ab["reads"], "aligned_aa": ab["aligned"], "rpkg": rpkg(ab["reads"], length_aa, ge),
             "sampled_reads": sampled, "trimmed_length": L, "ags": ags, "ags_source": source, "genome_equivalents_sampled": ge, "reads_assigned": ab["assigned"]}
    if mixed:
        table.update({"length_classes": list(classes), "class_reads": class_reads, "class_reads_assigned": class_assigned, "sampled_bases": bases})
    if fs is not None:
        table["long_genes"] = {"genes_split": args["gene_fold"]["genes_split"], "segments": len(args["gene_fold"]["seg_names"]), "edge_rows": fs["edge_rows"]}
        args["gene_fold_ms"] = fs["ms"]
    if cov is not None:
        breadth, mean_depth = coverage_columns(length_aa, cov["covered"], cov["spanned"])
        table.update({"covered_aa": cov["covered"], "breadth": breadth, "mean_depth": mean_depth, "max_depth": cov["max_depth"], "spanned_aa": cov["spanned"]})
        if args["min_breadth"] is not None:
            table.update({"min_breadth": args["min_breadth"], "detected": detect(ab["reads"], cov["covered"], length_aa, args["min_breadth"])})
        if counts["depth"] is not None:
            table["depth"] = counts["depth"]
    if ti is not None:
        sh = shared_reads(ti["share"])
        table.update({"unique_reads": ti["unique"], "candidate_reads": ti["candidates"], "shared_reads": sh, "rpkg_shared": rpkg(sh, length_aa, ge), "share": ti["share"],
                      "reads_ambiguous": ti["ambiguous"]})
        if tcov is not None:
            table.update({"covered_any_aa": tcov["covered_any"], "breadth_any": coverage_columns(length_aa, tcov["covered_any"], tcov["spanned_any"])[0]})
            if args["min_breadth"] is not None:
                table["detected_any"] = detect(ti["candidates"], tcov["covered_any"], length_aa, args["min_breadth"])
        if group_of is not None:
            table.update({"reads_ambiguous_across_groups": ti["group_ambiguous"], "group_unique": ti["group_unique"], "groups_ties": group_ties_table(
                counts["gids"], len(counts["gnames"]), ti["group_unique"], ti["share"], table["rpkg_shared"], table.get("detected_any"))})
    if gb is not None:
        se, lo, hi = boot_columns(gb["stats"], gb["used"], length_aa)
        table.update({"rpkg_boot_se": se, "rpkg_ci95_low": lo, "rpkg_ci95_high": hi, "boot_used": gb["used"], "boot_stats": gb["stats"], "boot_scale": counts["scale"],
                      "bootstrap": args["bootstrap"], "bootstrap_seed": args["bootstrap_seed"] or 0, "bootstrap_denominator": "replicate_ags" if est else "fixed_ags"})
    if group_of is not None:
        table["groups"] = group_table(names, table["reads"], table["rpkg"], group_of, table.get("detected"))
    tb = counts.get("tb")                                          # (a record from before the switch has no such key)
    if tb is not None:
        se, lo, hi = boot_columns(tb["stats"], tb["used"], length_aa)
        table.update({"rpkg_shared_boot_se": se, "rpkg_shared_ci95_low": lo, "rpkg_shared_ci95_high": hi, "tie_boot_stats": tb["stats"], "tie_boot_used": tb["used"],
                      "tie_list_entries": counts["tie_list"][0], "tie_list_capacity": counts["tie_list"][1]})
    cb = counts.get("cb")                                          # (a record from before the switch has no such key)
    if cb is not None:
        table.update(zip(COV_BOOT_COLUMNS, cov_boot_columns(cb["stats"], args["bootstrap"], length_aa)))
        table["cov_boot_stats"] = cb["stats"]
        if cb.get("detected") is not None:
            table.update({"cov_boot_detected": cb["detected"], "detected_support": np.asarray(cb["detected"], np.float64) / float(args["bootstrap"])})
    idn = counts.get("idn")                                        # (a record from before the switch has no such key)
    if idn is not None:
        table.update(identity_columns(idn, ab["reads"], ab["aligned"], length_aa, ge))
        table.update({"identity": idn, "ident_levels": list(idn["levels"])})
        if group_of is not None:
            table["groups_ident"] = group_ident_table(names, group_of, table)
    ds = counts.get("ds")                                          # (a record from before the switch has no such key)
    if ds is not None:                                              # whole-sample figures of the genes: nothing of them enters the groups or the curve
        table.update(depth_stat_columns(ds, counts.get("ds_any"), length_aa, ge))
        table.update({"depth_stats": ds, "tad_keep": int(ds["keep"])})
        if counts.get("ds_any") is not None:
            table["depth_stats_any"] = counts["ds_any"]
    gbg = counts.get("gbg")                                        # (a record from before the switch has no such key)
    if gbg is not None:                                           # (group_ids numbers the groups in group_table's order)
        table.update({"groups_boot": list(zip(*(col.tolist() for col in group_boot_columns(gbg["stats"], gbg["used"])))), "groups_boot_stats": gbg["stats"]})
    if cu is not None:
        points = [int(n) for n in counts["points"]]
        if cu["beyond"] != 0:
            raise AbundanceError("the curve: %d assigned reads lie behind the last point %d (%d sampled)" % (cu["beyond"], points[-1], sampled))
        ags_k = [ags] * len(points)
        if est:
            est_curve = pargs.get("ags_curve") or []
            if [p["reads"] for p in est_curve] != points:
                raise AbundanceError("the AGS curve's points %s are not the gene curve's %s" % ([p["reads"] for p in est_curve], points))
            ags_k = [p["ags"] for p in est_curve]
        table["curve"] = curve_figures(names, length_aa, L, points, cu["reads"], cu["aligned"], cu.get("covered"), ags_k, args["min_breadth"], group_of)
    return table


def write_outputs(args, table):
    """Stage 4 - the files: the depth file; the identity histogram; under outfile the gene, groups and curve tables; the curve's per-gene matrix"""
    if table.get("depth") is not None:
        write_depth(args["depth_out"], table["gene"], table["length_aa"], table["depth"])
    if table.get("identity") is not None and args.get("ident_out") is not None:
        write_ident(args["ident_out"], table["gene"], table["identity"]["hist"])
    if args.get("outfile"):
        write_table(args["outfile"], args, table)
        if "groups" in table:
            write_groups(args["outfile"] + ".groups.tsv", args, table)
        if "curve" in table:
            write_curve(args["outfile"] + ".curve.tsv", args, table)
    if "curve" in table and args["curve_genes"] is not None:
        write_curve_genes(args["curve_genes"], table)


def run_abundance(args):
    """args: run_pipeline's keys (seqfiles, nreads, read_length, min_quality, mean_quality, filter_dups, max_unknown, device, model_dir,
    verbose, outfile) plus genes, min_ident, min_aln, min_bits, groups, ags, ags_report and the switches the module's docstring describes,
    all off by default: coverage, min_breadth and depth_out (a path; both imply coverage), ties, curve (K, 1 .. 64: table['curve']; writes
    <outfile>.curve.tsv) with curve_genes (a path: the curve's per-gene matrix), bootstrap (B, 1 .. 4096) with bootstrap_seed (default 0; not
    combined with curve) and bootstrap_groups (needs bootstrap and groups: table['groups_boot'], one (se, low, high) per row of table['groups'],
    table['groups_boot_stats'], and the three columns behind every column of <outfile>.groups.tsv) and bootstrap_ties (needs bootstrap and ties:
    rpkg_shared_boot_se, rpkg_shared_ci95_low, rpkg_shared_ci95_high behind every column of the gene table, table['tie_boot_stats'] and
    table['tie_boot_used']; tie_list_factor, 1 .. 500, default 4, sizes its list; leaves args['tie_bootstrap_ms']) and bootstrap_coverage (needs
    bootstrap and coverage: breadth_boot_mean, breadth_boot_se, breadth_ci95_low, breadth_ci95_high and, with min_breadth, detected_support behind
    every column of the gene table, table['cov_boot_stats'] - six doubles per gene, in residues - and table['cov_boot_detected']; leaves
    args['coverage_bootstrap_ms']), mixed_lengths (True or a list of class lengths; not combined with read_length and curve, with bootstrap only under a
    given AGS), long_genes (genes of up to 65,535 residues; table['long_genes'] = {genes_split, segments, edge_rows}), identity with ident_levels (a
    list of 1 .. 8 ascending integer percents) and ident_out (a path; both imply identity: matched_aa, mismatched_aa, gap_opens, ident_mean,
    ident_median, ident_min, ident_max and per level reads_ident_ge<T>, rpkg_ident_ge<T> behind every column of the gene table, matched_aa,
    ident_mean and the levels' columns behind every column of <outfile>.groups.tsv, table['identity'] - Engine.identity()'s arrays -; leaves
    args['identity_ms']), depth_stats with tad_keep (P, an integer percent 1 .. 100, default 80; it implies depth_stats, both imply coverage:
    median_depth, tad<P> and tad<P>_per_ge behind every column of the gene table, identity's included, with ties median_depth_any and tad<P>_any;
    table['depth_stats'] - Engine.depth_stats()'s arrays -, table['tad_keep']; the groups, curve and depth files are what they are without it;
    leaves args['depth_stats_ms']).  Four stages with two
    records between them - DESIGN.md 13, "How a run is laid out on the host".  Writes args['outfile'] (and <outfile>.groups.tsv with groups)
    when it is set; leaves in args the sampler's options as imputed, sampled_reads, search_ms and the *_ms of every switch that ran; returns
    (table, args) - table: the columns as arrays, the header's values, and 'groups' [(group, genes, reads, rpkg)] with a map."""
    names, seqs, group_of, ags, source = check_request(args)
    microbe_census.check_input(args)
    sample = resolve_sample(args, ags, source)
    counts = device_pass(args, sample, names, seqs, group_of)
    table = build_table(args, sample, counts, names, seqs, group_of)
    write_outputs(args, table)
    return table, args
