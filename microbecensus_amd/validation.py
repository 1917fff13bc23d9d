"""How good is a model: mock communities of known composition, their simulated metagenomes, and the error of the AGS estimate
against the truth - the reference's own yardstick (tests/data/community.txt + metagenome.fa.gz, test_microbe_census.py: < 1 %;
optimize_weights.R: mue), with the metagenomes made and searched on the GPU (mc_community_library).

    genomes_dir/*.fna.gz + community files (genome, abundance) or --random K  --copies-->  communities of M genomes x copies
    per (community, read length): one fused pass of n reads  --best hits-->  aggregate_hits + _ags_of_sums  -->  est_ags vs true_ags

A community is M member genomes with an integer number of copies (cells) each; a read comes from member m with probability
proportional to copies[m] x (valid starts of m) (csrc/mc_simlib.h).  Its true AGS is exact:
sum(copies[m] x size[m]) / sum(copies[m]), size = the sum of the member's contig lengths.  The estimate is run_pipeline's: the same
aggregate_hits and _ags_of_sums on the best hits, with bases = reads x L.
"""
import decimal
import math
import os

import numpy as np

from . import training

COPIES_TOTAL = 1000000                       # copies = floor(a / sum(a) x COPIES_TOTAL + 0.5)
MAX_MEMBERS, MAX_COPIES = 65536, 1 << 20     # mc_community_open's limits
RANDOM_TAG = 0x6D635F636F6D6D                # "mc_comm": the key domain of the random communities' draws
ABUNDANCE_COLUMNS = ("relative_abundance", "abundance")


class ValidationError(ValueError):
    """A validation run refused before any GPU work."""


# ---- communities ------------------------------------------------------------------------------------------------------------
def _ratio(a, who):
    """(numerator, denominator) of an abundance, exactly: a decimal string as written, a float as it is."""
    try:
        if isinstance(a, str):
            d = decimal.Decimal(a.strip())
            if not d.is_finite():
                raise ValueError
            num, den = d.as_integer_ratio()
        else:
            f = float(a)
            if not math.isfinite(f):
                raise ValueError
            num, den = f.as_integer_ratio()
    except (ValueError, decimal.InvalidOperation, OverflowError):
        raise ValidationError("%s: abundance %r is not a finite number" % (who, a))
    if num < 0:
        raise ValidationError("%s: abundance %s is negative" % (who, a))
    return num, den


def copies_of(names, abundances):
    """copies[m] = floor(a[m] / sum(a) x 1,000,000 + 0.5) in integer arithmetic.  Refused by name: a negative or non-finite
    abundance, a member that comes to 0 copies or to more than the engine takes."""
    ratios = [_ratio(a, n) for n, a in zip(names, abundances)]
    den = 1
    for _, d in ratios:
        den = den * d // math.gcd(den, d)
    scaled = [num * (den // d) for num, d in ratios]
    total = sum(scaled)
    if total <= 0:
        raise ValidationError("the abundances sum to 0")
    copies = [(2 * s * COPIES_TOTAL + total) // (2 * total) for s in scaled]
    for n, k in zip(names, copies):
        if k < 1:
            raise ValidationError("%s comes to 0 copies of %d (its abundance is too small)" % (n, COPIES_TOTAL))
        if k > MAX_COPIES:
            raise ValidationError("%s comes to %d copies; a member has at most %d" % (n, k, MAX_COPIES))
    return copies


def true_ags_fraction(copies, sizes):
    """(numerator, denominator) of sum(copies x size) / sum(copies)."""
    return sum(int(k) * int(s) for k, s in zip(copies, sizes)), sum(int(k) for k in copies)


def true_ags(copies, sizes):
    num, den = true_ags_fraction(copies, sizes)
    return num / den                                # (int / int: correctly rounded)


def read_community(path, genome_names):
    """(members, abundances as written) of a community file: TSV with a header line; the first column is the genome's name, the
    abundance the column headed relative_abundance or abundance; other columns are ignored."""
    known = set(genome_names)
    with open(path) as f:
        lines = [ln.rstrip("\r\n") for ln in f if ln.strip()]
    if not lines:
        raise ValidationError("community file %s is empty" % path)
    head = [h.strip() for h in lines[0].split("\t")]
    col = [i for i, h in enumerate(head) if h in ABUNDANCE_COLUMNS and i > 0]
    if not col:
        raise ValidationError("community file %s has no column headed %s" % (path, " or ".join(ABUNDANCE_COLUMNS)))
    names, abund = [], []
    for ln in lines[1:]:
        x = ln.split("\t")
        name = x[0].strip()
        if len(x) <= col[0]:
            raise ValidationError("community file %s: the line of %s has no abundance" % (path, name))
        if name not in known:
            raise ValidationError("community file %s: no genome file for %s" % (path, name))
        if name in names:
            raise ValidationError("community file %s names %s twice" % (path, name))
        names.append(name)
        abund.append(x[col[0]].strip())
    if not names:
        raise ValidationError("community file %s names no genome" % path)
    return names, abund


def community_name(path):
    base = os.path.basename(path)
    return base[: base.rindex(".")] if "." in base else base


def random_community(genome_names, k, members, sigma, seed):
    """Community k of a --random run: `members` distinct genomes and log-normal(0, sigma) abundances from
    numpy.random.Generator(PCG64(SeedSequence([RANDOM_TAG, seed, k]))) - reproducible from (seed, k) alone.  (names in genome
    order, abundances as floats)."""
    if not 1 <= members <= len(genome_names):
        raise ValidationError("--members %d: there are %d genomes" % (members, len(genome_names)))
    if not (sigma >= 0 and math.isfinite(sigma)):
        raise ValidationError("--sigma %s must be a finite number >= 0" % sigma)
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([RANDOM_TAG, int(seed) & 0xFFFFFFFFFFFFFFFF, int(k)])))
    pick = np.sort(rng.choice(len(genome_names), size=int(members), replace=False))
    abund = rng.lognormal(0.0, float(sigma), size=int(members))
    return [genome_names[i] for i in pick.tolist()], [float(a) for a in abund.tolist()]


def parse_length_mix(text):
    """--length-mix 100:0.5,150:0.5 -> [(100, 0.5), (150, 0.5)], ascending: the length classes of a mixed library and the share of
    its reads each holds.  Refused: anything else, a length twice, a share that is not positive, shares that do not add up to 1."""
    mix = []
    try:
        for item in text.split(","):
            L, share = item.split(":")
            mix.append((int(L), float(share)))
    except ValueError:
        raise ValidationError("--length-mix %s: expected L1:share1,L2:share2,..." % text)
    if len(set(L for L, _ in mix)) != len(mix):
        raise ValidationError("--length-mix %s names a length twice" % text)
    if any(not (s > 0 and math.isfinite(s)) for _, s in mix):
        raise ValidationError("--length-mix %s: every share must be positive" % text)
    if abs(sum(s for _, s in mix) - 1.0) > 1e-9:
        raise ValidationError("--length-mix %s: the shares add up to %s, not 1" % (text, sum(s for _, s in mix)))
    return sorted(mix)


def mix_label(length_mix):
    return "+".join(str(L) for L, _ in length_mix)


def check_request(read_lengths, nreads, valid_lengths, where, error_model=None, error_rate=None, paired_end=False, insert=None, reference_lengths=False, length_mix=None):
    """Every refusal of a validation run that needs no genome, before any GPU work."""
    if reference_lengths:
        raise ValidationError("a community library has reads of one length: the reference read lengths (--reference-lengths) are not supported")
    if not read_lengths and not length_mix:
        raise ValidationError("no read length given (-l)")
    read_lengths = list(read_lengths) + [L for L, _ in length_mix or []]
    if length_mix and paired_end and any(round(s * nreads) % 2 for _, s in length_mix):
        raise ValidationError("a paired-end library has an even number of reads: --length-mix gives a class an odd number of -n %d" % nreads)
    for L in read_lengths:
        if L not in valid_lengths:
            raise ValidationError("read length %s is not one the model %s was trained for: %s" % (L, where, list(valid_lengths)))
    if nreads < 1:
        raise ValidationError("reads per library (-n) must be positive")
    if nreads > 0x7FFFFFFF:
        raise ValidationError("reads per library (-n) must stay below 2^31")
    if error_model is not None and error_model not in training.ERROR_MODELS:
        raise ValidationError("unknown error model %r (illumina or uniform)" % (error_model,))
    if error_model == "uniform" and error_rate is None:
        raise ValidationError("the uniform error model needs an error rate (--error-rate)")
    if error_rate is not None and error_model != "uniform":
        raise ValidationError("an error rate (--error-rate) goes only with the uniform error model")
    if error_rate is not None and not 0 <= error_rate <= 1:
        raise ValidationError("error rate %s outside [0, 1]" % error_rate)
    if paired_end and insert is None:
        raise ValidationError("a paired-end library needs an insert (--insert)")
    if insert is not None and not paired_end:
        raise ValidationError("an insert (--insert) goes only with a paired-end library (--paired-end)")
    if paired_end and insert < max(read_lengths):
        raise ValidationError("insert %d is shorter than the read length %d" % (insert, max(read_lengths)))
    if paired_end and nreads % 2:
        raise ValidationError("a paired-end library has an even number of reads (-n %d)" % nreads)


def unsigned_error_summary(records):
    """{read length: (median, maximum) of |error|} over the records that have an estimate (optimize_weights.R: mue)."""
    out = {}
    for L in sorted(set(r["read_length"] for r in records), key=lambda L: (isinstance(L, str), L)):      # (a --length-mix row: "100+150")
        e = [abs(r["error"]) for r in records if r["read_length"] == L and r["error"] is not None]
        out[L] = (float(np.median(e)), float(max(e))) if e else (None, None)
    return out


# ---- the run ------------------------------------------------------------------------------------------------------------------
def estimate_of_best_hits(model_dir, read_length, best, families, nreads):
    """run_pipeline's estimate of a library of nreads reads of read_length from its best hits: aggregate_hits, then _ags_of_sums
    with bases = reads x L.  None when no read was classified or no family survives."""
    from . import microbe_census as mc
    if len(best) == 0:
        return None
    args = {"model_dir": model_dir, "read_length": read_length, "verbose": False}
    agg = mc.aggregate_hits(args, {}, mc._BestHits(best, families))
    return mc._ags_or_none(mc._model(model_dir), read_length, agg, nreads * read_length)


def estimate_of_mixed_passes(model_dir, length_mix, counts, bests, families):
    """run_pipeline's mixed-lengths estimate of a library made of one pass per length class: per class aggregate_hits over its best
    hits, pooled by pooled_ags.  None when no read was classified or no family survives."""
    from . import microbe_census as mc
    sums = [mc.aggregate_hits({"model_dir": model_dir, "read_length": L, "verbose": False}, {}, mc._BestHits(b, families)) if len(b) else {}
            for (L, _), b in zip(length_mix, bests)]
    # (_ags_or_none's conditions: no bases, no family with a hit, or none that survives the outlier cut)
    if sum(n * L for n, (L, _) in zip(counts, length_mix)) <= 0 or not any(v != 0 for s in sums for v in s.values()):
        return None
    try:
        return mc.pooled_ags(mc._model(model_dir), [L for L, _ in length_mix], counts, sums)
    except ZeroDivisionError:
        return None


def validate(genomes_dir, out_dir, read_lengths, nreads, model_dir=None, communities=None, random=0, members=None, sigma=1.0, seed=0, device=0,
             error_model=None, error_rate=None, paired_end=False, insert=None, write_reads_dir=None, reference_lengths=False, log=print, length_mix=None):
    """Scores a model on mock communities.  communities: community files; random: how many random communities (of `members`
    genomes, log-normal(0, sigma) abundances).  Writes out_dir/validation.map and out_dir/communities/<name>.tsv and returns the
    records: dicts of community, read_length, members, reads, true_ags, est_ags (None without a classified read), error (signed,
    relative; None likewise) and member_reads."""
    from . import _native
    from . import microbe_census as mc
    read_lengths = [int(L) for L in read_lengths]
    nreads = int(nreads)
    if model_dir:
        mc.check_model_dir(model_dir)
    check_request(read_lengths, nreads, mc._valid_read_lengths(model_dir), model_dir or "(packaged)", error_model, error_rate, paired_end, insert, reference_lengths, length_mix)
    label = mix_label(length_mix) if length_mix else None
    genomes = training.list_genomes(genomes_dir)
    names = [g for g, _ in genomes]
    if not communities and not random:
        raise ValidationError("no community given (--communities FILE ... or --random K)")
    wanted = []                                      # (name, members, abundances)
    for path in communities or []:
        wanted.append((community_name(path),) + read_community(path, names))
    for k in range(int(random or 0)):
        if members is None:
            raise ValidationError("--random needs --members")
        wanted.append(("random%03d" % k,) + random_community(names, k, int(members), float(sigma), seed))
    if len(set(w[0] for w in wanted)) != len(wanted):
        raise ValidationError("two communities have the same name")
    plan = []
    for cname, mem, abund in wanted:
        if len(mem) > MAX_MEMBERS:
            raise ValidationError("community %s has %d members; at most %d" % (cname, len(mem), MAX_MEMBERS))
        plan.append((cname, mem, copies_of(mem, abund)))
    path_of = dict(genomes)
    loaded = {}
    for _, mem, _ in plan:
        for g in mem:
            if g not in loaded:
                loaded[g] = _native.read_fasta_genome(path_of[g])
    span = insert if paired_end else max(read_lengths + [L for L, _ in length_mix or []])
    for cname, mem, _ in plan:
        if not any(len(loaded[g][1]) > 1 and int(np.max(np.diff(loaded[g][1]))) >= span for g in mem):
            raise ValidationError("community %s has no contig of at least %d bp" % (cname, span))
    model = mc._model(model_dir)
    fams = model["families"]
    log("Validating %s on %d communities, read lengths %s, %d reads per library" % ("the model in %s" % model_dir if model_dir else "the packaged model", len(plan), read_lengths, nreads))
    eng = mc._engines_on([device], model_dir)[0]
    os.makedirs(os.path.join(out_dir, "communities"), exist_ok=True)
    records = []
    for cname, mem, copies in plan:
        sizes = [int(loaded[g][1][-1]) for g in mem]
        truth = true_ags(copies, sizes)
        comm = _native.Community([loaded[g] for g in mem], copies, device)
        drawn = {}
        try:
            comm.set_library(error_model, error_rate, paired_end, insert)
            for L in read_lengths:
                eng.set_run(L, model["pars"][str(L)], fams)
                lid = training.library_id(cname, L)
                best = eng.community_library(comm, nreads, seed, lid)
                drawn[L] = comm.member_reads()
                est = estimate_of_best_hits(model_dir, L, best, fams, nreads)
                rec = {"community": cname, "read_length": L, "members": len(mem), "reads": nreads, "true_ags": truth, "est_ags": est,
                       "error": None if est is None else (est - truth) / truth, "member_reads": drawn[L].tolist()}
                records.append(rec)
                log("  %s L=%d: true %.2f, estimated %s, error %s" % (cname, L, truth, "NA" if est is None else "%.2f" % est,
                                                                     "NA" if est is None else "%+.4f" % rec["error"]))
                if write_reads_dir:
                    training.write_reads(os.path.join(write_reads_dir, "%s_%d.fa.gz" % (cname, L)), comm.simulate(L, nreads, seed, lid), paired_end)
            if length_mix:
                # a library of mixed lengths: one pass per class with round(share x n) reads and a library id of its own, the passes
                # combined as run_pipeline's mixed_lengths combines the classes of a file
                counts, bests = [], []
                drawn[label] = np.zeros(len(mem), np.int64)
                for L, share in length_mix:
                    n_k = int(round(share * nreads))
                    counts.append(n_k)
                    if n_k == 0:
                        bests.append(np.zeros(0, _native.BEST_DTYPE))
                        continue
                    eng.set_run(L, model["pars"][str(L)], fams)
                    lid = training.library_id("%s|%s" % (cname, label), L)
                    bests.append(eng.community_library(comm, n_k, seed, lid))
                    drawn[label] += comm.member_reads()
                    if write_reads_dir:                            # the mixed library, one file per class
                        training.write_reads(os.path.join(write_reads_dir, "%s_%s_%d.fa.gz" % (cname, label, L)), comm.simulate(L, n_k, seed, lid), paired_end)
                est = estimate_of_mixed_passes(model_dir, length_mix, counts, bests, fams)
                rec = {"community": cname, "read_length": label, "members": len(mem), "reads": sum(counts), "true_ags": truth, "est_ags": est,
                       "error": None if est is None else (est - truth) / truth, "member_reads": drawn[label].tolist(), "class_reads": counts}
                records.append(rec)
                log("  %s L=%s: true %.2f, estimated %s, error %s" % (cname, label, truth, "NA" if est is None else "%.2f" % est, "NA" if est is None else "%+.4f" % rec["error"]))
        finally:
            comm.close()
        with open(os.path.join(out_dir, "communities", cname + ".tsv"), "w") as f:
            cols = read_lengths + ([label] if length_mix else [])
            f.write("\t".join(["genome", "copies", "size"] + ["reads_%s" % L for L in cols]) + "\n")
            for i, g in enumerate(mem):
                f.write("\t".join([g, str(copies[i]), str(sizes[i])] + [str(int(drawn[L][i])) for L in cols]) + "\n")
    summary = unsigned_error_summary(records)
    with open(os.path.join(out_dir, "validation.map"), "w") as f:
        f.write("\t".join(["community", "read_length", "members", "reads", "true_ags", "est_ags", "error"]) + "\n")
        for r in records:
            f.write("\t".join([r["community"], str(r["read_length"]), str(r["members"]), str(r["reads"]), repr(r["true_ags"]),
                               "NA" if r["est_ags"] is None else repr(r["est_ags"]), "NA" if r["error"] is None else repr(r["error"])]) + "\n")
        for L, (med, worst) in summary.items():
            line = "read length %s: median unsigned error %s, maximum %s" % (L, "NA" if med is None else "%.4f" % med, "NA" if worst is None else "%.4f" % worst)
            f.write("# " + line + "\n")
            log(line)
    return records
