"""The cases that hold run_abundance's files to recorded bytes (tests/golden/abundance_tables.json), defined once: what every case asks
for, the inputs it is run on, the hash of a file it writes, and how the records between run_abundance's stages (sample, counts) go into
and come out of tests/golden/abundance_tables.npz.  tests/golden/make_abundance_tables_golden.py, test_abundance_table_host.py and
test_gpu_abundance_tables.py share it; test_gpu_abund_classes_e2e.py and test_gpu_fold.py take their inputs' recipes from here."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HASHES = os.path.join(GOLD, "abundance_tables.json")
RECORDS = os.path.join(GOLD, "abundance_tables.npz")
CLASSES = [100, 150]
AGS = 3.0e6

# case: (options, the inputs other than the example FASTQ and the packaged markers)
CASES = {
    "plain": (dict(ags=AGS), ()),
    "full": (dict(ags=AGS, coverage=True, min_breadth=0.1, ties=True), ("groups", "depth_out")),
    "curve": (dict(ags=AGS, min_breadth=0.1, curve=3), ("groups", "curve_genes")),
    "boot_fixed": (dict(ags=AGS, coverage=True, bootstrap=32, bootstrap_seed=7), ()),
    "boot_own": (dict(bootstrap=32, bootstrap_seed=7), ()),                          # no AGS: run_pipeline estimates it, replicate by replicate
    "mixed": (dict(ags=AGS, mixed_lengths=list(CLASSES), coverage=True, ties=True), ("mixed_reads",)),
    "long": (dict(ags=AGS, long_genes=True, coverage=True), ("joined_genes",)),      # no ties: under a fold shared_reads depends on the row order at 2^-32
}
# the header lines that hold the paths of the machine the run was on
PATH_LINES = (b"# metagenome:", b"# genes:", b"# groups:")
# what build_table reads of run_pipeline's args: the rest of them (paths, threads, times) does not go into the fixture
SAMPLE_PARGS = ("file_type", "quality_offset", "read_length", "nreads", "min_quality", "mean_quality", "filter_dups", "max_unknown", "sampled_reads", "length_classes",
                "class_reads", "ags_curve", "ags_boot_se", "ags_ci95", "ags_boot_replicates", "ags_boot_values", "ags_boot_reads")
# the parts of `counts` that are None where a case does not ask for them
COUNTS_OR_NONE = ("ac", "cov", "depth", "ti", "tcov", "cu", "points", "gb", "scale", "fold_stats", "gids", "gnames")


def write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, s.decode()))
    return str(path)


def mixed_reads():
    """(reads, lengths): 30,000 reads of 40 - 320 bp off a synthetic community of the packaged markers (test_gpu_classes.py's recipe)"""
    from microbecensus_amd import _native, synth
    _, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=1_500_000, seed=31, marker_gene_fraction=0.3)
    full = synth.sample_reads(genome, 30_000, 320, seed=32)
    lens = np.random.default_rng(33).integers(40, 321, size=len(full))
    return [bytes(full[i, :lens[i]]) for i in range(len(full))], lens


def group_map(names):
    """the first 4,000 genes grouped by their names' prefix (the family), every other gene a group of its own"""
    return {n: n.split("_")[0] for n in names[:4000]}


def long_gene_markers():
    """every second packaged marker: the database the long-gene tests cut and join (test_gpu_fold.py says why not all of them)"""
    from microbecensus_amd import _native
    names, seqs = _native.load_markers()
    return names[::2], seqs[::2]


def pick_joined(seqs, unique):
    """the three markers of about 1,000 residues with the most unique reads (unique: Engine.ties()['unique'] of the example reads)"""
    return [int(g) for g in np.argsort(-np.asarray(unique)) if 800 <= len(seqs[g]) <= 1183][:3]


def write_joined_genes(path, names, seqs, order):
    """a FASTA of the gene `joined` - the markers `order` one after the other - and then every other marker; returns (path, joined, the others)"""
    joined = "".join(seqs[g] for g in order)
    keep = [g for g in range(len(names)) if g not in order]
    with open(path, "w") as f:
        for nm, sq in zip(["joined"] + [names[g] for g in keep], [joined] + [seqs[g] for g in keep]):
            f.write(">%s\n%s\n" % (nm, sq))
    return str(path), joined, keep


def request(case, d, reads=True):
    """run_abundance's args for a case, its inputs written under the directory d.  reads=False: the reads of `mixed` are not made (the
    stages behind the device pass never open them)."""
    from microbecensus_amd import _native
    options, inputs = CASES[case]
    d = str(d)
    args = dict({"seqfiles": [os.path.join(GOLD, "inputs", "example.fq.gz")], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "nreads": 10000, "device": 0,
                 "outfile": os.path.join(d, case + ".tsv")}, **options)
    if "groups" in inputs:
        args["groups"] = os.path.join(d, "map.tsv")
        with open(args["groups"], "w") as f:
            f.write("".join("%s\t%s\n" % kv for kv in group_map(_native.load_markers()[0]).items()))
    if "depth_out" in inputs:
        args["depth_out"] = os.path.join(d, case + ".depth")
    if "curve_genes" in inputs:
        args["curve_genes"] = os.path.join(d, case + ".curve_genes.tsv")
    if "mixed_reads" in inputs:
        args["seqfiles"] = [write_fasta(os.path.join(d, "mixed.fa"), mixed_reads()[0]) if reads else os.path.join(d, "mixed.fa")]
    if "joined_genes" in inputs:
        names, seqs = long_gene_markers()
        order = [names.index(nm) for nm in recorded()["long_joined"]]
        args["genes"] = write_joined_genes(os.path.join(d, "joined.faa"), names, seqs, order)[0]
    return args


def files_of(args):
    """{what: path} of the files a run of these args writes"""
    out = {"table": args["outfile"]}
    if args.get("groups"):
        out["groups"] = args["outfile"] + ".groups.tsv"
    if args.get("curve"):
        out["curve"] = args["outfile"] + ".curve.tsv"
    if args.get("curve_genes"):
        out["curve_genes"] = args["curve_genes"]
    if args.get("depth_out"):
        out["depth"] = args["depth_out"]
    return out


def file_hash(path):
    """SHA-256 of a file without its PATH_LINES"""
    with open(path, "rb") as f:
        return hashlib.sha256(b"".join(line for line in f if not line.startswith(PATH_LINES))).hexdigest()


def hashes_of(args):
    return {what: file_hash(path) for what, path in files_of(args).items()}


def recorded():
    with open(HASHES) as f:
        return json.load(f)


def expected():
    return recorded()["cases"]


# ---- the records between the stages, in one .npz: <case>/sample a JSON text, <case>/counts/<key>[/<key>] arrays ---------------------
def _plain(v):
    return v.tolist() if isinstance(v, (np.ndarray, np.generic)) else v


def pack(case, sample, counts, into):
    s = dict(sample, pargs={k: sample["pargs"][k] for k in SAMPLE_PARGS if k in sample["pargs"]})
    into[case + "/sample"] = np.array(json.dumps(s, default=_plain, sort_keys=True))

    def walk(prefix, v):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(prefix + "/" + k, x)
        elif v is not None:
            into[prefix] = np.asarray(v)
    walk(case + "/counts", counts)


def unpack(npz, case):
    """(sample, counts) as the stages hand them on: arrays, ints and floats, lists of names, None for what the case did not ask for"""
    sample = json.loads(str(npz[case + "/sample"]))
    counts = dict.fromkeys(COUNTS_OR_NONE)
    for key in npz.files:
        if key.startswith(case + "/counts/"):
            at, path, v = counts, key.split("/")[2:], npz[key]
            for k in path[:-1]:
                at[k] = at = at.get(k) or {}
            at[path[-1]] = v.item() if v.ndim == 0 else v.tolist() if v.dtype.kind == "U" else v
    return sample, counts


def same_counts(a, b, where="counts"):
    """the differences between two counts records, the times aside: a list of key paths"""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)):
            return [where]
        return [w for k in sorted(set(a) | set(b)) if not k.endswith("_ms") and k != "ms" for w in same_counts(a.get(k), b.get(k), where + "/" + k)]
    if a is None or b is None:
        return [] if a is None and b is None else [where]
    a, b = np.asarray(a), np.asarray(b)
    return [] if a.shape == b.shape and a.dtype.kind == b.dtype.kind and a.tobytes() == np.asarray(b, a.dtype).tobytes() else [where]
