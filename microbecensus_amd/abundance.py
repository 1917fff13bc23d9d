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

Reads of mixed lengths (mixed_lengths; README "Reads of mixed lengths"): one trimmed length drops every shorter read and the tail of
every longer one.  Under the switch every read is searched and counted at the largest length class L_k it reaches
(Engine.set_abundance_classes; csrc/k_abund_classes.h states the rule), and the denominator is that of the bases so sampled:

    sampled_bases = sum over the classes of n_k x L_k       genome_equivalents_sampled = sampled_bases / AGS

n_k the reads of class k, counted on the device beside the reads each class assigned.  The default AGS is run_pipeline's estimate
under the same classes: numerator and denominator still come from the same sampled bases."""
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
BOOT_COLUMNS = ("rpkg_boot_se", "rpkg_ci95_low", "rpkg_ci95_high")                  # behind all of them with bootstrap
MAX_BOOT = 4096                                                                      # MC_GB_MAXB (csrc/mc_geneboot.h)
MAX_CURVE = 64                                                                       # MC_CURVE_MAXK (csrc/mc_curve.h)
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


def _mixed_header(table):
    if table.get("length_classes") is None:
        return []
    return [(k, ",".join(str(int(x)) for x in table[k])) for k in ("length_classes", "class_reads", "class_reads_assigned")] + [("sampled_bases", table["sampled_bases"])]


def header_lines(args, table):
    h = [("metagenome", ",".join(args["seqfiles"])), ("genes", args["genes"]), ("sampled_reads", table["sampled_reads"]),
         ("trimmed_length", table["trimmed_length"])] + _mixed_header(table) + [("min_ident", args["min_ident"]), ("min_aln", args["min_aln"]), ("min_bits", repr(float(args["min_bits"]))),
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


def write_table(path, args, table):
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        boot = table.get("rpkg_boot_se") is not None
        if boot:                                                   # (the gene table's alone: the groups table does not bootstrap)
            out.writelines("# %s:\t%s\n" % kv for kv in (("bootstrap", table["bootstrap"]), ("bootstrap_seed", table["bootstrap_seed"]),
                                                         ("bootstrap_replicates", "%d/%d" % (table["boot_used"], table["bootstrap"])),
                                                         ("bootstrap_denominator", table["bootstrap_denominator"])))
        cov, det = table.get("covered_aa") is not None, table.get("detected") is not None
        ties, tcov, tdet = table.get("unique_reads") is not None, table.get("covered_any_aa") is not None, table.get("detected_any") is not None
        out.write("\t".join(COLUMNS + (COVERAGE_COLUMNS if cov else ()) + (("detected",) if det else ()) + (TIES_COLUMNS if ties else ())
                            + (TIES_COVERAGE_COLUMNS if tcov else ()) + (("detected_any",) if tdet else ()) + (BOOT_COLUMNS if boot else ())) + "\n")
        for k, (nm, ln, r, a, v) in enumerate(zip(table["gene"], table["length_aa"], table["reads"], table["aligned_aa"], table["rpkg"])):
            line = "%s\t%d\t%d\t%d\t%s" % (nm, ln, r, a, repr(float(v)))
            if cov:
                line += "\t%d\t%s\t%s\t%d" % (table["covered_aa"][k], repr(float(table["breadth"][k])), repr(float(table["mean_depth"][k])), table["max_depth"][k])
            if det:
                line += "\t%d" % table["detected"][k]
            if ties:
                line += "\t%d\t%d\t%s\t%s" % (table["unique_reads"][k], table["candidate_reads"][k], repr(float(table["shared_reads"][k])), repr(float(table["rpkg_shared"][k])))
            if tcov:
                line += "\t%d\t%s" % (table["covered_any_aa"][k], repr(float(table["breadth_any"][k])))
            if tdet:
                line += "\t%d" % table["detected_any"][k]
            if boot:
                line += "\t%s\t%s\t%s" % tuple(repr(float(table[c][k])) for c in BOOT_COLUMNS)
            out.write(line + "\n")


def write_groups(path, args, table):
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        out.write("# groups:\t%s\n" % args["groups"])
        det = table.get("detected") is not None
        gt = table.get("groups_ties")
        tdet = gt is not None and table.get("detected_any") is not None
        out.write("\t".join(GROUP_COLUMNS + (("genes_detected",) if det else ()) + (GROUP_TIES_COLUMNS if gt is not None else ()) + (("genes_detected_any",) if tdet else ())) + "\n")
        for k, row in enumerate(table["groups"]):
            g, n, r, v = row[:4]
            more = ""
            if gt is not None:
                more = "\t%d\t%s\t%s" % (gt[k][0], repr(float(gt[k][1])), repr(float(gt[k][2]))) + ("\t%d" % gt[k][3] if tdet else "")
            out.write("%s\t%d\t%d\t%s%s%s\n" % (g, n, r, repr(float(v)), "\t%d" % row[4] if det else "", more))


def _na(v, fmt=repr):
    return "NA" if v is None else fmt(v)


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
    det, grp = "genes_detected" in cu, "groups_with_reads" in cu
    with open(path, "w") as out:
        out.writelines(header_lines(args, table))
        out.write("\t".join(CURVE_COLUMNS + (("genes_detected",) if det else ()) + (("groups_with_reads",) if grp else ())) + "\n")
        for k, n_k in enumerate(cu["points"]):
            line = "%d\t%s\t%s\t%d\t%d" % (n_k, _na(cu["ags"][k]), _na(cu["genome_equivalents_sampled"][k]), cu["reads_assigned"][k], cu["genes_with_reads"][k])
            out.write(line + ("\t%d" % cu["genes_detected"][k] if det else "") + ("\t%d" % cu["groups_with_reads"][k] if grp else "") + "\n")


def write_curve_genes(path, table):
    """--curve-genes: gene, reads_1 .. reads_K and with coverage covered_aa_1 .. covered_aa_K - genes in FASTA order"""
    cu = table["curve"]
    K, cov = len(cu["points"]), cu.get("covered_aa")
    with open(path, "w") as out:
        out.write("# curve_points:\t%s\n" % "\t".join(str(n) for n in cu["points"]))
        out.write("\t".join(["gene"] + ["reads_%d" % (k + 1) for k in range(K)] + (["covered_aa_%d" % (k + 1) for k in range(K)] if cov is not None else [])) + "\n")
        for g, nm in enumerate(table["gene"]):
            out.write("\t".join([nm] + [str(int(cu["reads"][k, g])) for k in range(K)] + ([str(int(cov[k, g])) for k in range(K)] if cov is not None else [])) + "\n")


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


PIPELINE_KEYS = ("seqfiles", "nreads", "read_length", "min_quality", "mean_quality", "filter_dups", "max_unknown", "threads", "device", "model_dir", "verbose")


def _pipeline_args(args):
    # (nreads None is run_pipeline's "no cap" and is handed on; any other key that is None is left to impute_missing_args)
    return {k: (list(args[k]) if k == "seqfiles" else args[k]) for k in PIPELINE_KEYS if k in args and (args[k] is not None or k == "nreads")}


def check_request(args):
    """Everything that can be refused before any GPU work; returns (names, seqs, group_of, ags or None, ags_source or None)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.get("distributed"):
        raise AbundanceError("Gene abundances are not computed by a distributed run (WORLD_SIZE %s): run one process" % os.environ.get("WORLD_SIZE", "1"))
    for key, default in (("min_ident", 0), ("min_aln", 0), ("min_bits", 0.0), ("groups", None), ("ags", None), ("ags_report", None),
                         ("coverage", False), ("min_breadth", None), ("depth_out", None), ("ties", False), ("curve", None), ("curve_genes", None),
                         ("bootstrap", None), ("bootstrap_seed", None), ("mixed_lengths", None), ("long_genes", False)):
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
        K = args["curve"]
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= MAX_CURVE:
            raise AbundanceError("--curve %s is not an integer from 1 to %d" % (K, MAX_CURVE))
        args["curve"] = int(K)
    if args["bootstrap"] is not None:
        B = args["bootstrap"]
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= int(B) <= MAX_BOOT:
            raise AbundanceError("--bootstrap %s is not an integer from 1 to %d" % (B, MAX_BOOT))
        args["bootstrap"] = int(B)
        if args["curve"] is not None:
            raise AbundanceError("--bootstrap %d cannot be combined with --curve %d: the curve's points are not bootstrapped" % (args["bootstrap"], args["curve"]))
    if args["bootstrap_seed"] is not None:
        S = args["bootstrap_seed"]
        if args["bootstrap"] is None:
            raise AbundanceError("--bootstrap-seed %s needs --bootstrap B: it seeds the replicates" % (S,))
        if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 0 <= int(S) < 1 << 64:
            raise AbundanceError("--bootstrap-seed %s is not an integer from 0 to 2^64 - 1" % (S,))
        args["bootstrap_seed"] = int(S)
    if args["curve_genes"] is not None:
        if not args["curve_genes"]:
            raise AbundanceError("--curve-genes %r is an empty path" % (args["curve_genes"],))
        if args["curve"] is None:
            raise AbundanceError("--curve-genes %s needs --curve K: it writes the curve's per-gene matrix" % (args["curve_genes"],))
        where = os.path.abspath(args["curve_genes"])
        others = [(args.get("outfile"), "the gene table itself"), (args["outfile"] + ".curve.tsv" if args.get("outfile") else None, "the curve table (<outfile>.curve.tsv)"),
                  (args["outfile"] + ".groups.tsv" if args.get("outfile") and args["groups"] else None, "the groups table (<outfile>.groups.tsv)"),
                  (args["depth_out"] or None, "the depth file (--depth-out)")]
        for other, what in others:
            if other and where == os.path.abspath(other):
                raise AbundanceError("--curve-genes %s is the path of %s: two files" % (args["curve_genes"], what))
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
        where = os.path.abspath(args["depth_out"])
        if args.get("outfile") and where == os.path.abspath(args["outfile"]):
            raise AbundanceError("--depth-out %s is the path of the gene table itself: two files" % (args["depth_out"],))
        if args.get("outfile") and args["groups"] and where == os.path.abspath(args["outfile"] + ".groups.tsv"):
            raise AbundanceError("--depth-out %s is the path of the groups table (<outfile>.groups.tsv): two files" % (args["depth_out"],))
    if not isinstance(args["ties"], (bool, int)) or args["ties"] not in (0, 1):
        raise AbundanceError("ties %r is not a switch: True or False" % (args["ties"],))
    args["ties"] = bool(args["ties"])
    args["coverage"] = bool(args["coverage"]) or args["min_breadth"] is not None or args["depth_out"] is not None
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
    ags = source = None
    if args["ags"] is not None:
        source = "--ags"
        ags = check_ags(args["ags"], source)
    if not isinstance(args["long_genes"], (bool, int)) or args["long_genes"] not in (0, 1):
        raise AbundanceError("long_genes %r is not a switch: True or False" % (args["long_genes"],))
    args["long_genes"] = bool(args["long_genes"])
    names, seqs = read_genes(args["genes"], args["long_genes"])
    args["gene_fold"] = split_genes(names, seqs) if args["long_genes"] else None      # (refused here: before any GPU work)
    group_of = read_groups(args["groups"], names) if args["groups"] else None
    if args["ags_report"] is not None:
        source = "report %s" % args["ags_report"]
        ags = check_ags(read_ags_report(args["ags_report"]), source)
    if mixed:                   # (None: to be detected from the reads, once the files are known to be there)
        args["length_classes"] = resolve_length_classes(args, list(microbe_census._valid_read_lengths(args.get("model_dir"))))
    return names, seqs, group_of, ags, source


def run_abundance(args):
    """args: run_pipeline's keys (seqfiles, nreads, read_length, min_quality, mean_quality, filter_dups, max_unknown, device, model_dir,
    verbose, outfile) plus genes, min_ident, min_aln, min_bits, groups, ags, ags_report and - all off by default - mixed_lengths (True or a list of class lengths: every read
    at the largest length class it reaches, the denominator from the bases so sampled; not combined with read_length and curve, with bootstrap only under a given AGS), coverage, min_breadth
    (implies coverage), depth_out (a path; implies coverage), ties (the genes that tie for a read's best hit: unique, candidate and
    shared reads beside the counts; sets args['ties_ms']), curve (K, 1 .. 64: table['curve'], the table's figures at K prefixes of the sample
    - the sampler then runs to its end before the search starts; sets args['curve_ms']; writes <outfile>.curve.tsv) and curve_genes (a path:
    the curve's per-gene matrix), bootstrap (B, 1 .. 4096: the columns rpkg_boot_se, rpkg_ci95_low, rpkg_ci95_high from B Poisson-bootstrap
    replicates of the sampled reads under bootstrap_seed (default 0) - with run_pipeline's AGS every replicate is divided by its own
    genome equivalents, with a given AGS by the fixed ones; sets args['gene_bootstrap_ms']; not combined with curve), long_genes (genes of up to
    65,535 residues: split_genes cuts the long ones into overlapping segments, the engine folds every row back onto its gene, every table is the genes';
    table['long_genes'] = {genes_split, segments, edge_rows}; sets args['gene_fold_ms']).  Writes args['outfile'] (and
    <outfile>.groups.tsv with groups) when it is set; returns (table, args) - table: the columns as arrays (gene, length_aa, reads,
    aligned_aa, rpkg), the header's values, and 'groups' [(group, genes, reads, rpkg)] with a map."""
    names, seqs, group_of, ags, source = check_request(args)
    microbe_census.check_input(args)
    mixed, classes = microbe_census.mixed_lengths_on(args), None
    if mixed:                   # neither a list nor a report's line: the classes run_pipeline would detect on the same file
        classes = args["length_classes"]
        if classes is None:
            try:
                classes = microbe_census.auto_detect_length_classes(args["seqfiles"][0], list(microbe_census._valid_read_lengths(args.get("model_dir"))))
            except SystemExit as e:
                raise AbundanceError(str(e))
        args["length_classes"] = classes = [int(x) for x in classes]
    if ags is None:             # the estimate of the same sample: run_pipeline on the marker engine, same files, same options
        more = {"curve": args["curve"]} if args["curve"] else {"bootstrap": args["bootstrap"], "bootstrap_seed": args["bootstrap_seed"] or 0} if args["bootstrap"] else {}
        if mixed:               # (check_request has refused the curve and the bootstrap of a default AGS)
            more = {"mixed_lengths": list(classes)}
        est = microbe_census.run_pipeline(dict(_pipeline_args(args), **more) if more else _pipeline_args(args))
        if est is None:
            raise AbundanceError("run_pipeline gave no AGS estimate for %s" % ",".join(args["seqfiles"]))
        ags, pargs = est
        source = "run_pipeline"
        ags = check_ags(ags, source)
    else:                       # the same imputation run_pipeline makes (file type, quality offset, read length), without a search
        pargs = _pipeline_args(args)
        microbe_census._cap_host_threads(pargs.get("threads"))
        if mixed:               # (as run_pipeline: read_length becomes "mixed" and is not detected)
            pargs["mixed_lengths"] = list(classes)
            microbe_census.check_mixed_lengths(pargs)
        microbe_census.impute_missing_args(pargs)
        microbe_census.check_arguments(pargs)
    L = "mixed" if mixed else int(pargs["read_length"])
    sampler = (pargs["nreads"], pargs["file_type"] == "fastq", pargs.get("quality_offset") or 0, pargs["min_quality"], pargs["mean_quality"], pargs["max_unknown"], pargs["filter_dups"])
    rd = _native.Reader.with_classes(pargs["seqfiles"], classes, *sampler) if mixed else _native.Reader(pargs["seqfiles"], L, *sampler)
    eng = None
    try:
        fold = args["gene_fold"]
        if fold is None:
            eng = _native.Engine(device=int(args.get("device") or 0), names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1)
        else:                   # long_genes: the engine on the segments with the genes' statistics, every table below in gene space
            eng = _native.Engine(device=int(args.get("device") or 0), names=fold["seg_names"], seqs=fold["seg_seqs"], marker_family=[0] * len(fold["seg_names"]), nfam=1, stats=fold["stats"])
            eng.set_gene_fold(fold["seg_gene"], fold["seg_off"], fold["gene_len"])
        if mixed:               # (the default parameters: classification does not enter the counts)
            eng.set_run_classes(classes)
        else:
            eng.set_run(L)
        eng.set_abundance(True, min_ident=args["min_ident"], min_aln=args["min_aln"], min_bits=args["min_bits"])
        if args["coverage"]:
            eng.set_coverage(True)
        gids = None
        if args["ties"]:
            if group_of is not None:
                gids, gnames = group_ids(names, group_of)
                eng.set_ties(True, gids, len(gnames))
            else:
                eng.set_ties(True)
        if mixed:
            eng.set_abundance_classes(True)
        cu = points = gb = scale = ac = None
        B, seed = args["bootstrap"], args["bootstrap_seed"] or 0
        if B and pargs["nreads"] is not None:       # ids lie below -n: the list is sized before the sampler starts, and it samples beside the search
            eng.set_gene_bootstrap(int(pargs["nreads"]))
        try:
            if B and pargs["nreads"] is None:       # no cap: the list's size is the number of reads the sampler takes - it runs to its end first
                n = rd.run()
                if n:
                    eng.set_gene_bootstrap(n)
                    eng.lib.mc_set_keep_rows(eng.h, 0)
                    try:
                        if mixed:
                            eng.search_classes(rd.reads(n))
                        else:
                            eng.search(rd.reads(n))
                    finally:
                        eng.lib.mc_set_keep_rows(eng.h, 1)
            elif args["curve"]:       # the points depend on how many reads the sampler takes: it runs to its end first, then one search
                n = rd.run()
                if n:               # (no read taken: nothing is searched, and the run ends below with "No reads remaining after filtering" as without the switch)
                    points = microbe_census.curve_points(n, args["curve"])
                    eng.set_curve(points)
                    eng.lib.mc_set_keep_rows(eng.h, 0)
                    try:
                        eng.search(rd.reads(n))
                    finally:
                        eng.lib.mc_set_keep_rows(eng.h, 1)
                    cu = eng.curve(covered=bool(args["coverage"]))
                    args["curve_ms"] = eng.curve_ms()
            else:
                eng.search_files(rd, keep_rows=False)
        except _native.ReferenceError_ as e:
            raise AbundanceError(str(e))
        ab = eng.abundance()
        if mixed:
            ac = eng.abundance_classes()
            args["abundance_classes_ms"] = eng.abundance_classes_ms()
        if B and ab["searched"]:
            if source == "run_pipeline":
                if len(pargs.get("ags_boot_values") or []) != B or len(pargs.get("ags_boot_reads") or []) != B:
                    raise AbundanceError("run_pipeline gave %d replicate AGS values for --bootstrap %d" % (len(pargs.get("ags_boot_values") or []), B))
                scale = boot_scale(pargs["ags_boot_values"], pargs["ags_boot_reads"], L)
            else:
                scale = np.full(B, 1.0 / (sampled_bases(ac["rows"], classes) / ags if mixed else genome_equivalents(ab["searched"], L, ags)))
            try:
                gb = eng.gene_bootstrap(B, seed, scale)
            except RuntimeError as e:
                raise AbundanceError(str(e))
            args["gene_bootstrap_ms"] = eng.gene_bootstrap_ms()
        cov = eng.coverage() if args["coverage"] else None
        depth = eng.coverage_depth() if args["depth_out"] is not None else None
        args["abundance_ms"], args["search_ms"] = eng.abundance_ms(), eng.stats()["ms_total"]
        ti = eng.ties() if args["ties"] else None
        tcov = eng.ties_coverage() if args["ties"] and args["coverage"] else None
        if args["coverage"]:
            args["coverage_ms"] = eng.coverage_ms()
        if args["ties"]:
            args["ties_ms"] = eng.ties_ms()
        fs = eng.gene_fold_stats() if fold is not None else None
        st = rd.stats()
    finally:
        rd.close()
        if eng is not None:
            eng.close()
    sampled = int(st["sampled"])
    if sampled == 0:
        raise AbundanceError("No reads remaining after filtering")
    if "sampled_reads" in pargs and int(pargs["sampled_reads"]) != sampled or ab["searched"] != sampled:
        raise AbundanceError("the gene search saw %d reads (%d sampled), the AGS estimate %s" % (ab["searched"], sampled, pargs.get("sampled_reads")))
    class_reads = class_assigned = None
    if mixed:
        K = len(classes)
        class_reads, class_assigned = [int(x) for x in ac["rows"][:K]], [int(x) for x in ac["assigned"][:K]]
        est = source == "run_pipeline"
        if sum(class_reads) != sampled or int(ac["rows"][K]) != 0 or est and (list(pargs.get("length_classes") or []) != classes or list(pargs.get("class_reads") or []) != class_reads):
            raise AbundanceError("the gene search saw %d reads (%d sampled): %s reads in the classes %s and %d below them, the AGS estimate %s in the classes %s"
                                 % (ab["searched"], sampled, class_reads, classes, int(ac["rows"][K]), pargs.get("class_reads") if est else "-", pargs.get("length_classes") if est else "-"))
        args["class_reads"] = class_reads
    for k in ("file_type", "quality_offset", "read_length", "nreads", "min_quality", "mean_quality", "filter_dups", "max_unknown") + (
            ("ags_boot_se", "ags_ci95", "ags_boot_replicates", "ags_boot_values", "ags_boot_reads") if gb is not None and source == "run_pipeline" else ()):
        if k in pargs:
            args[k] = pargs[k]
    args["sampled_reads"] = sampled
    length_aa = np.array([len(s) for s in seqs], np.int64)
    bases = sampled_bases(class_reads, classes) if mixed else None
    ge = bases / ags if mixed else genome_equivalents(sampled, L, ags)
    table = {"gene": list(names), "length_aa": length_aa, "reads": ab["reads"], "aligned_aa": ab["aligned"], "rpkg": rpkg(ab["reads"], length_aa, ge),
             "sampled_reads": sampled, "trimmed_length": L, "ags": ags, "ags_source": source, "genome_equivalents_sampled": ge, "reads_assigned": ab["assigned"]}
    if mixed:
        table.update({"length_classes": list(classes), "class_reads": class_reads, "class_reads_assigned": class_assigned, "sampled_bases": bases})
    if fs is not None:
        table["long_genes"] = {"genes_split": fold["genes_split"], "segments": len(fold["seg_names"]), "edge_rows": fs["edge_rows"]}
        args["gene_fold_ms"] = fs["ms"]
    if cov is not None:
        breadth, mean_depth = coverage_columns(length_aa, cov["covered"], cov["spanned"])
        table.update({"covered_aa": cov["covered"], "breadth": breadth, "mean_depth": mean_depth, "max_depth": cov["max_depth"], "spanned_aa": cov["spanned"]})
        if args["min_breadth"] is not None:
            table["min_breadth"] = args["min_breadth"]
            table["detected"] = detect(ab["reads"], cov["covered"], length_aa, args["min_breadth"])
        if depth is not None:
            table["depth"] = depth
            write_depth(args["depth_out"], names, length_aa, depth)
    if ti is not None:
        sh = shared_reads(ti["share"])
        table.update({"unique_reads": ti["unique"], "candidate_reads": ti["candidates"], "shared_reads": sh, "rpkg_shared": rpkg(sh, length_aa, ge), "share": ti["share"],
                      "reads_ambiguous": ti["ambiguous"]})
        if tcov is not None:
            table.update({"covered_any_aa": tcov["covered_any"], "breadth_any": coverage_columns(length_aa, tcov["covered_any"], tcov["spanned_any"])[0]})
            if args["min_breadth"] is not None:
                table["detected_any"] = detect(ti["candidates"], tcov["covered_any"], length_aa, args["min_breadth"])
        if group_of is not None:
            table["reads_ambiguous_across_groups"] = ti["group_ambiguous"]
            table["group_unique"] = ti["group_unique"]
            table["groups_ties"] = group_ties_table(gids, len(gnames), ti["group_unique"], ti["share"], table["rpkg_shared"], table.get("detected_any"))
    if gb is not None:
        se, lo, hi = boot_columns(gb["stats"], gb["used"], length_aa)
        table.update({"rpkg_boot_se": se, "rpkg_ci95_low": lo, "rpkg_ci95_high": hi, "boot_used": gb["used"], "boot_stats": gb["stats"], "boot_scale": scale, "bootstrap": B,
                      "bootstrap_seed": seed, "bootstrap_denominator": "replicate_ags" if source == "run_pipeline" else "fixed_ags"})
    if group_of is not None:
        table["groups"] = group_table(names, table["reads"], table["rpkg"], group_of, table.get("detected"))
    if cu is not None:
        if cu["beyond"] != 0:
            raise AbundanceError("the curve: %d assigned reads lie behind the last point %d (%d sampled)" % (cu["beyond"], points[-1], sampled))
        if source == "run_pipeline":
            est_curve = pargs.get("ags_curve") or []
            if [p["reads"] for p in est_curve] != points:
                raise AbundanceError("the AGS curve's points %s are not the gene curve's %s" % ([p["reads"] for p in est_curve], points))
            ags_k = [p["ags"] for p in est_curve]
        else:
            ags_k = [ags] * len(points)
        table["curve"] = curve_figures(names, length_aa, L, points, cu["reads"], cu["aligned"], cu.get("covered"), ags_k, args["min_breadth"], group_of)
    if args.get("outfile"):
        write_table(args["outfile"], args, table)
        if group_of is not None:
            write_groups(args["outfile"] + ".groups.tsv", args, table)
        if cu is not None:
            write_curve(args["outfile"] + ".curve.tsv", args, table)
    if cu is not None and args["curve_genes"] is not None:
        write_curve_genes(args["curve_genes"], table)
    return table, args
