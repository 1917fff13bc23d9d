"""Training a model: the reference's training/ workflow (TRAINING.txt steps 1 - 4) with simulation, search and grid
classification on the GPU (mc_train_library) and the parameter fit of optimize_parameters.py on the host.

    genomes_dir/*.fna.gz  --simulate (seq_sim.py --cov [-e -r] [-p -i]), search (-e 1), grid-classify-->  per-family counts
    counts / library bp   --x-fold cross-validation (training.py:71-169)-->  pars.map, coefficients.map, ...  + model.json

Two orders the reference leaves to chance are fixed here: genomes are taken in sorted name order (the reference: os.listdir
order, which decides the folds), and the candidates of one (read length, family) are enumerated min_score ascending, then
max_pid ascending, then aln_cov ascending, then rate type hits / aln / cov - the FIRST strict minimum of the cross-validation
error wins (the reference: whichever of its parallel processes finished first).  Weights are 1.0 for every (read length, family)
unless fit_weights is set: then step 5 (optimize_weights.R) runs as the device's candidate search (fit_weights(), csrc/mc_wfit.h).

Libraries are single end without errors by default; error_model ('uniform' at error_rate, or 'illumina') and paired_end (with an
insert) give seq_sim.py's other kinds (csrc/mc_simlib.h), with one deviation by default: every read keeps exactly L bases.
reference_lengths=True (--reference-lengths) gives seq_sim.py's reads of L + insertions - deletions bases instead: each is searched
at its own length (mc_search_varlen's buckets) and a library's bp is their real total, the reference's rate denominator.
"""
import glob
import gzip
import json
import math
import os
import zlib

import numpy as np

# the grid of class_reads.py:51-53
ALN_COVS = [0.0, 0.25, 0.5, 0.75]
MAX_PIDS = [50, 60, 70, 80, 90, 100]
MIN_SCORES = list(range(23, 50))
RATE_TYPES = ("hits", "aln", "cov")
MIN_READ_LEN, MAX_READ_LEN = 18, 510          # what the engine searches (mc_set_run)
MAX_FAMILIES, MAX_MARKERS = 32, 32767          # the engine's limits
ERROR_MODELS = ("illumina", "uniform")


class TrainingError(ValueError):
    """A training run refused before any GPU work."""


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _listing(directory, ext, what):
    if not os.path.isdir(directory):
        raise TrainingError("%s directory %s does not exist" % (what, directory))
    files = sorted(f for f in os.listdir(directory) if not f.startswith("."))
    if not files:
        raise TrainingError("%s directory %s is empty" % (what, directory))
    bad = [f for f in files if not f.endswith(ext)]
    if bad:
        raise TrainingError("%s must have %s extension: %s" % (what, ext, ", ".join(bad[:5])))
    return [(f[: -len(ext)], os.path.join(directory, f)) for f in files]


def list_genomes(genomes_dir):
    """[(name, path)] of genomes_dir/*.fna.gz in sorted name order (name = file stem)."""
    return _listing(genomes_dir, ".fna.gz", "Genomes")


def list_families(gene_fams_dir):
    """[(family, path)] of gene_fams_dir/*.faa.gz in sorted order (family = file stem)."""
    return _listing(gene_fams_dir, ".faa.gz", "Gene family files")


def _fasta_records(path):
    opener = gzip.open if path.endswith(".gz") else open
    name, chunks = None, []
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    yield name, "".join(chunks)
                name, chunks = line[1:].split()[0], []
            else:
                chunks.append(line.strip())
    if name is not None:
        yield name, "".join(chunks)


def build_marker_set(families):
    """(names, seqs, marker_family, family_names) from [(family, path)]: files in the given (sorted) order, records in file order,
    the first occurrence of each distinct sequence kept - the rule the packaged markers.faa.gz was built by."""
    seen = set()
    names, seqs, fam_of = [], [], []
    fam_names = [f for f, _ in families]
    for fi, (_, path) in enumerate(families):
        for name, seq in _fasta_records(path):
            if seq in seen:
                continue
            seen.add(seq)
            names.append(name)
            seqs.append(seq)
            fam_of.append(fi)
    return names, seqs, fam_of, fam_names


def packaged_marker_set():
    from . import _native
    names, seqs = _native.load_markers()
    model = _native.load_model()
    return names, seqs, list(model["marker_family"]), list(model["families"])


def py2_round(x):
    """Python 2's round(x): halves away from zero (seq_sim.py sizes a library with it)."""
    y = math.floor(abs(x))
    r = y + 1.0 if abs(x) - y >= 0.5 else y
    return math.copysign(r, x)


def library_reads(coverage, genome_size, read_len):
    """n = round(cov x G / L) (seq_sim.py:79); the library holds n x L bp (library_sizes)."""
    return int(py2_round(coverage * genome_size / float(read_len)))


def library_id(genome_name, read_len):
    """The library of one genome at one read length: a stable id, independent of which other genomes are trained with it."""
    return (int(read_len) << 32) | zlib.crc32(genome_name.encode())


def library_record(error_model=None, error_rate=None, paired_end=False, insert=None, reference_lengths=False):
    """model.json's "library" record of a library kind; None for the default (single end, no errors, reads of L bases)."""
    if error_model is None and not paired_end and not reference_lengths:
        return None
    rec = {"error_model": error_model, "error_rate": error_rate, "paired_end": bool(paired_end), "insert": insert if paired_end else None}
    if reference_lengths:
        rec["reference_lengths"] = True
    return rec


def check_request(genomes, read_lengths, xfolds, coverage, n_families, n_markers, error_model=None, error_rate=None, paired_end=False, insert=None):
    """Every refusal of a training run, before any GPU work."""
    if not read_lengths:
        raise TrainingError("no read length given (-l)")
    for L in read_lengths:
        if not MIN_READ_LEN <= L <= MAX_READ_LEN:
            raise TrainingError("read length %s outside %d..%d" % (L, MIN_READ_LEN, MAX_READ_LEN))
    if xfolds < 1:
        raise TrainingError("cross-validation folds (-x) must be at least 1")
    if xfolds > len(genomes):
        raise TrainingError("%d-fold cross-validation needs at least %d genomes; %d given" % (xfolds, xfolds, len(genomes)))
    if not coverage > 0:
        raise TrainingError("coverage (-c) must be positive")
    if n_families > MAX_FAMILIES:
        raise TrainingError("%d gene families: the engine takes at most %d" % (n_families, MAX_FAMILIES))
    if n_markers > MAX_MARKERS:
        raise TrainingError("%d marker sequences: the engine takes at most %d" % (n_markers, MAX_MARKERS))
    if n_markers == 0:
        raise TrainingError("the gene family files hold no sequences")
    if error_model is not None and error_model not in ERROR_MODELS:
        raise TrainingError("unknown error model %r (illumina or uniform)" % (error_model,))
    if error_model == "uniform" and error_rate is None:
        raise TrainingError("the uniform error model needs an error rate (--error-rate)")
    if error_rate is not None and error_model != "uniform":
        raise TrainingError("an error rate (--error-rate) goes only with the uniform error model")
    if error_rate is not None and not 0 <= error_rate <= 1:
        raise TrainingError("error rate %s outside [0, 1]" % error_rate)
    if paired_end and insert is None:
        raise TrainingError("a paired-end library needs an insert (--insert)")
    if insert is not None and not paired_end:
        raise TrainingError("an insert (--insert) goes only with a paired-end library (--paired-end)")
    if paired_end and insert < max(read_lengths):
        raise TrainingError("insert %d is shorter than the read length %d" % (insert, max(read_lengths)))


# ---- the fit (optimize_parameters.py, training.py:71-169) --------------------------------------------------------------------
def xfold_indexes(n, x, i):
    """training.py:100-115 with integer fold size n // x: genomes behind x * (n // x) are never in a test fold."""
    fold = n // x
    test = list(range(fold * i - fold, fold * i))
    return [j for j in range(n) if j not in test], test


def xval_errors(rates, sizes, xfolds):
    """Cross-validation median percent error of every candidate.  rates: (genomes, candidates); sizes: (genomes,).  An error of 999
    where a test genome's rate is 0 (test_error)."""
    rates = np.asarray(rates, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.float64)
    n = rates.shape[0]
    errs = []
    for i in range(1, xfolds + 1):
        train, test = xfold_indexes(n, xfolds, i)
        pc = np.median(sizes[train, None] * rates[train], axis=0)        # estimate_proportionality_constant
        for j in test:
            r = rates[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                e = 100 * np.abs(pc / r - sizes[j]) / sizes[j]
            errs.append(np.where(r == 0, 999.0, e))
    return np.median(np.array(errs), axis=0)


def candidates():
    """(min_score, max_pid, aln_cov, rate_type) in the order the fit walks them."""
    return [(s, p, c, t) for s in MIN_SCORES for p in MAX_PIDS for c in ALN_COVS for t in RATE_TYPES]


def rates_by_candidate(hits, aln, cov, library_bp):
    """Per-genome count arrays of shape (aln_cov, max_pid, min_score, family) -> rates (genomes, family, candidates) in the order of
    candidates()."""
    r = np.stack([np.asarray(hits, np.float64), np.asarray(aln, np.float64), np.asarray(cov, np.float64)], axis=-1)   # (G, c, p, s, f, t)
    r = r / np.asarray(library_bp, np.float64)[:, None, None, None, None, None]
    r = r.transpose(0, 4, 3, 2, 1, 5)                                        # (G, f, s, p, c, t)
    return r.reshape(r.shape[0], r.shape[1], -1)


def fit(rates, sizes, xfolds):
    """rates: (genomes, candidates) of one (read length, family).  Returns (index of the chosen candidate, its error, coefficient,
    predictions, every candidate's error): the first strict minimum of the cross-validation error; the coefficient is the median
    over ALL genomes of size x rate; a prediction is coefficient / rate, None where the rate is 0."""
    rates = np.asarray(rates, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.float64)
    err = xval_errors(rates, sizes, xfolds)
    k = int(np.argmin(err))                                                  # (first occurrence of the minimum)
    rk = rates[:, k]
    coeff = float(np.median([s * r for s, r in zip(sizes.tolist(), rk.tolist())]))
    preds = [coeff / r if r > 0 else None for r in rk.tolist()]
    return k, float(err[k]), coeff, preds, err


# ---- step 5: the per-family weights (optimize_weights.R as a device candidate search) -------------------------------------------
def weight_tables(preds_rows, families, read_lengths):
    """{L: (pred (N, F) float64 with NaN for NA, truth (N,), genome names)} from rows shaped as training_preds.map's: (read_length,
    fam, genome_name, true_ags, est_ags), values as read from the file (strings, 'NA') or as train() holds them (numbers, None).
    Libraries in the order of their first row, families in the order given."""
    fidx = {f: i for i, f in enumerate(families)}
    out = {}
    for L in read_lengths:
        rows = [r for r in preds_rows if int(r[0]) == int(L)]
        genomes = list(dict.fromkeys(r[2] for r in rows))
        gidx = {g: i for i, g in enumerate(genomes)}
        pred = np.full((len(genomes), len(families)), np.nan)
        truth = np.zeros(len(genomes))
        for _, fam, g, true_ags, est in rows:
            truth[gidx[g]] = float(true_ags)
            if fam in fidx and est is not None and est != "NA":
                pred[gidx[g], fidx[fam]] = float(est)
        out[int(L)] = (pred, truth, genomes)
    return out


def fit_weights(preds_rows, families, read_lengths, engine, seed=0, candidates=None, generations=None):
    """TRAINING.txt step 5 on the device, one call of mc_fit_weights per read length.  Returns ({"<L>_<fam>": weight}, {L: (mue at
    1 / F, mue fitted)}).  engine: an open _native.Engine - there is no CPU fallback."""
    if engine is None or not getattr(engine, "h", None):
        raise RuntimeError("fit_weights searches its candidates on the GPU (mc_fit_weights) and there is no CPU fallback: no open engine given")
    weights, mues = {}, {}
    for L, (pred, truth, _) in weight_tables(preds_rows, families, read_lengths).items():
        if not len(truth):
            raise TrainingError("no training predictions for read length %d" % L)
        w, trace = engine.fit_weights(pred, truth, seed, L, candidates, generations)
        for fam, v in zip(families, w.tolist()):
            weights["%d_%s" % (L, fam)] = v
        mues[L] = (float(trace[0, 0]), float(trace[-1, 0]))
    return weights, mues


_fit_weights = fit_weights            # (train() has a switch of the same name)


def weights_fit_record(seed, candidates, generations, mues):
    """model.json's "weights_fit" record"""
    from . import _native
    return {"seed": int(seed), "candidates": int(candidates) if candidates else _native.WFIT_DEFAULT_C,
            "generations": _native.WFIT_DEFAULT_G if generations is None or generations < 0 else int(generations),
            "mue": {str(L): [m[0], m[1]] for L, m in sorted(mues.items())}}


def _fit_engine(device, names, seqs, marker_family, nfam):
    from . import _native
    try:
        return _native.Engine(device=device, names=names, seqs=seqs, marker_family=marker_family, nfam=nfam)
    except RuntimeError as e:
        raise RuntimeError("the weights are fitted on the GPU (mc_fit_weights) and there is no CPU fallback: %s" % e)


def refit_model_dir(model_dir, device=0, seed=0, candidates=None, generations=None, log=print):
    """Step 5 as a command of its own (scripts/optimize_weights.py): fits the weights on model_dir/training_preds.map and rewrites
    weights.map and the weights (and "weights_fit") of model.json.  Returns the model."""
    from . import _native
    path = os.path.join(model_dir, "training_preds.map")
    if not os.path.isfile(path):
        raise TrainingError("%s does not exist (a model directory written by train_microbe_census.py holds it)" % path)
    with open(os.path.join(model_dir, "model.json")) as f:
        model = json.load(f)
    names, seqs = _native.load_markers(os.path.join(model_dir, "markers.faa.gz"))
    eng = _fit_engine(device, names, seqs, model["marker_family"], len(model["families"]))
    try:
        weights, mues = fit_weights(read_map(path, header=True), model["families"], model["read_lengths"], eng, seed, candidates, generations)
    finally:
        eng.close()
    model["weights"] = weights
    model["weights_fit"] = weights_fit_record(seed, candidates, generations, mues)
    with open(os.path.join(model_dir, "model.json"), "w") as f:
        json.dump(model, f, separators=(",", ":"), sort_keys=True)
    write_weights_map(model_dir, weights)
    log(fit_log_line(model["weights_fit"]))
    return model


def fit_log_line(rec):
    return "Weights fitted on the GPU (seed %d, %d candidates x %d generations); median unsigned error per read length: %s" % (
        rec["seed"], rec["candidates"], rec["generations"], ", ".join("%s: %.4g -> %.4g" % (L, m[0], m[1]) for L, m in sorted(rec["mue"].items(), key=lambda kv: int(kv[0]))))


def write_weights_map(out_dir, weights):
    with open(os.path.join(out_dir, "weights.map"), "w") as f:
        for k in sorted(weights):
            f.write("%s\t%r\n" % (k, weights[k]))


# ---- outputs ------------------------------------------------------------------------------------------------------------------
def write_model(out_dir, names, seqs, marker_family, families, read_lengths, pars, coefficients, weights, genome_sizes=None, preds=None, library=None,
                weights_fit=None):
    """markers.faa.gz + model.json (the packaged schema, tools/build_data.py, plus the "library" record of a kind other than the
    default) and the reference's tables."""
    os.makedirs(out_dir, exist_ok=True)
    with gzip.GzipFile(os.path.join(out_dir, "markers.faa.gz"), "wb", mtime=0) as f:
        for name, seq in zip(names, seqs):
            f.write((">%s\n%s\n" % (name, seq)).encode())
    model = {"families": list(families), "marker_family": list(marker_family), "read_lengths": sorted(int(L) for L in read_lengths),
             "pars": pars, "coefficients": coefficients, "weights": weights}
    if library is not None:
        model["library"] = library
    if weights_fit is not None:
        model["weights_fit"] = weights_fit
    with open(os.path.join(out_dir, "model.json"), "w") as f:
        json.dump(model, f, separators=(",", ":"), sort_keys=True)
    with open(os.path.join(out_dir, "pars.map"), "w") as f:
        f.write("\t".join(["gene_fam", "read_length", "aln_cov", "max_pid", "min_score", "aln_stat"]) + "\n")
        for L in sorted(pars, key=int):
            for fam in sorted(pars[L]):
                cov, pid, score, stat = pars[L][fam]
                f.write("\t".join(str(x) for x in [fam, L, cov, pid, score, stat]) + "\n")
    with open(os.path.join(out_dir, "coefficients.map"), "w") as f:
        for k in sorted(coefficients):
            f.write("%s\t%r\n" % (k, coefficients[k]))
    write_weights_map(out_dir, weights)
    with open(os.path.join(out_dir, "read_len.map"), "w") as f:
        for L in sorted(int(L) for L in read_lengths):
            f.write("%d\n" % L)
    with open(os.path.join(out_dir, "gene_fam.map"), "w") as f:
        for name, fi in zip(names, marker_family):
            f.write("%s\t%s\n" % (name, families[fi]))
    with open(os.path.join(out_dir, "gene_len.map"), "w") as f:
        for name, seq in zip(names, seqs):
            f.write("%s\t%d\n" % (name, len(seq)))
    if preds is not None:
        with open(os.path.join(out_dir, "training_preds.map"), "w") as f:
            f.write("\t".join(["read_length", "fam", "genome_name", "true_ags", "est_ags"]) + "\n")
            for L, fam, genome, est in preds:
                f.write("%s\t%s\t%s\t%d\t%s\n" % (L, fam, genome, genome_sizes[genome], "NA" if est is None else repr(est)))
    return model


def read_map(path, header=False):
    """The rows of a .map table, split on tabs."""
    with open(path) as f:
        lines = f.read().splitlines()
    return [ln.split("\t") for ln in lines[1 if header else 0:] if ln]


def write_reads(path, reads, paired_end=False):
    """A library in seq_sim.py's format: '>id\\nseq\\n', ids 0, 1, ...; paired end: '>k/1', '>k/2' for rows 2k, 2k + 1.  reads: an
    (n, L) array, or (bases, offsets) of reads at their own lengths.  A path ending in .gz is written gzipped."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if isinstance(reads, tuple):
        bases, off = reads
        rows = (bases[off[i]:off[i + 1]] for i in range(len(off) - 1))
    else:
        rows = (reads[i] for i in range(reads.shape[0]))
    with (gzip.open(path, "wb", compresslevel=1) if path.endswith(".gz") else open(path, "wb")) as f:
        for i, row in enumerate(rows):
            f.write(b">%d/%d\n" % (i >> 1, 1 + (i & 1)) if paired_end else b">%d\n" % i)
            f.write(row.tobytes())
            f.write(b"\n")


def write_hits(path, families, hits, aln, cov):
    """A library's grid counts as class_reads.py writes them (.hits: fam, aln_cov, max_pid, min_score, count_hits, count_aln, count_cov)."""
    with open(path, "w") as f:
        f.write("\t".join(["fam", "aln_cov", "max_pid", "min_score", "count_hits", "count_aln", "count_cov"]) + "\n")
        for ic, c in enumerate(ALN_COVS):
            for ip, p in enumerate(MAX_PIDS):
                for isc, s in enumerate(MIN_SCORES):
                    for fi, fam in enumerate(families):
                        f.write("\t".join(str(x) for x in [fam, c, p, s, int(hits[ic, ip, isc, fi]), int(aln[ic, ip, isc, fi]), repr(float(cov[ic, ip, isc, fi]))]) + "\n")


# ---- the run ------------------------------------------------------------------------------------------------------------------
def train(genomes_dir, out_dir, read_lengths, coverage, gene_fams_dir=None, xfolds=10, seed=0, device=0, write_reads_dir=None, log=print,
          error_model=None, error_rate=None, paired_end=False, insert=None, reference_lengths=False, fit_weights=False, fit_seed=0, fit_candidates=None,
          fit_generations=None):
    """TRAINING.txt steps 1 - 4 in one call, and step 5 with fit_weights=True (the weights fitted on the device at fit_seed, with
    fit_candidates x fit_generations candidates; None: the defaults of csrc/mc_wfit.h).  reference_lengths: seq_sim.py's read lengths (L + insertions - deletions), the library's
    bp their real total.  A paired-end library at coverage c holds library_reads(c, G, L) pairs (seq_sim.py's
    read_id counts pairs), so twice as many reads; a library's bp is its reads x L either way.  Returns the model dict written to
    out_dir/model.json, with the run's rates under '_rates' ({L: (genomes, families, candidates)}) and the genomes' sizes under
    '_sizes'."""
    from . import _native
    read_lengths = [int(L) for L in read_lengths]
    genomes = list_genomes(genomes_dir)
    if gene_fams_dir:
        names, seqs, marker_family, families = build_marker_set(list_families(gene_fams_dir))
    else:
        names, seqs, marker_family, families = packaged_marker_set()
    check_request(genomes, read_lengths, xfolds, coverage, len(families), len(names), error_model, error_rate, paired_end, insert)
    library = library_record(error_model, error_rate, paired_end, insert, reference_lengths)
    loaded = []
    for gname, path in genomes:
        bases, off = _native.read_fasta_genome(path)
        longest = int(np.max(np.diff(off))) if len(off) > 1 else 0
        for L in read_lengths:
            span = insert if paired_end else L
            if longest < span:
                raise TrainingError("genome %s has no contig of at least %d bp" % (gname, span))
        loaded.append((gname, bases, off))
    sizes = {g: int(off[-1]) for g, _, off in loaded}
    size_list = [sizes[g] for g, _, _ in loaded]
    log("Training on %d genomes, %d gene families (%d markers), read lengths %s, %sx coverage, %d-fold cross-validation"
        % (len(loaded), len(families), len(names), read_lengths, coverage, xfolds))
    if library is not None:
        log("Library: %s" % ", ".join("%s %s" % kv for kv in sorted(library.items()) if kv[1] not in (None, False)))
    eng = (_fit_engine if fit_weights else _native.Engine)(device, names, seqs, marker_family, len(families))
    gpu_genomes = [_native.Genome(bases, off, device) for _, bases, off in loaded]
    if library is not None:
        for g in gpu_genomes:
            g.set_library(error_model, error_rate, paired_end, insert)
            if reference_lengths:
                g.set_read_lengths(True)
    cands = candidates()
    pars, coefficients, weights, preds, all_rates = {}, {}, {}, [], {}
    try:
        for L in read_lengths:
            eng.set_run(L)
            counts, lib_bp = [], []
            for (gname, _, _), g in zip(loaded, gpu_genomes):
                n = library_reads(coverage, sizes[gname], L) * (2 if paired_end else 1)
                lid = library_id(gname, L)
                hits, aln, cov = eng.train_library(g, n, seed, lid, ALN_COVS, MAX_PIDS, MIN_SCORES)
                counts.append((hits, aln, cov))
                lib_bp.append(eng.train_library_bases() if reference_lengths else n * L)
                if write_reads_dir:
                    reads = g.simulate_varlen(L, n, seed, lid) if reference_lengths else g.simulate(L, n, seed, lid)
                    write_reads(os.path.join(write_reads_dir, str(L), gname + "-reads.fa"), reads, paired_end)
                    write_hits(os.path.join(write_reads_dir, str(L), gname + ".hits"), families, hits, aln, cov)
                log("  L=%d %s: %d reads" % (L, gname, n))
            rates = rates_by_candidate([c[0] for c in counts], [c[1] for c in counts], [c[2] for c in counts], lib_bp)
            all_rates[L] = rates
            pars[str(L)] = {}
            for fi, fam in enumerate(families):
                k, _, coeff, pr, _ = fit(rates[:, fi, :], size_list, xfolds)
                s, p, c, t = cands[k]
                pars[str(L)][fam] = [float(c), float(p), float(s), t]
                coefficients["%d_%s" % (L, fam)] = coeff
                weights["%d_%s" % (L, fam)] = 1.0
                preds.extend((L, fam, gname, est) for (gname, _, _), est in zip(loaded, pr))
        fit_rec = None
        if fit_weights:
            weights, mues = _fit_weights([(L, fam, g, sizes[g], est) for L, fam, g, est in preds], families, read_lengths, eng, fit_seed, fit_candidates, fit_generations)
            fit_rec = weights_fit_record(fit_seed, fit_candidates, fit_generations, mues)
    finally:
        for g in gpu_genomes:
            g.close()
        eng.close()
    model = write_model(out_dir, names, seqs, marker_family, families, read_lengths, pars, coefficients, weights, sizes, preds, library, fit_rec)
    zero = sorted(k for k, v in coefficients.items() if v == 0)
    if zero:
        log("Families no genome's reads were assigned to (coefficient 0): %s" % ", ".join(zero))
    if fit_rec is not None:
        log(fit_log_line(fit_rec))
    else:
        log("Weights are not fitted (optimize_weights.R is out of scope): every read length and family has weight 1.0")
    log("Model written to %s" % out_dir)
    model["_rates"], model["_sizes"] = all_rates, sizes
    return model
