"""The Poisson bootstrap of csrc/mc_boot.h restated in numpy (uint64 arithmetic that wraps like the C code's): the weight of a read
in a replicate and the per-family sums of mc_bootstrap.  The threshold table is parsed out of the header, not typed again."""
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "microbecensus_amd", "csrc", "mc_boot.h")
GOLD = os.path.join(HERE, "golden")
U = np.uint64


def _header_constants():
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    key = int(re.search(r"#define\s+MC_BOOT_KEY\s+0x([0-9A-Fa-f]+)ull", text).group(1), 16)
    k = int(re.search(r"#define\s+MC_BOOT_K\s+(\d+)", text).group(1))
    body = re.search(r"MC_BOOT_THR\[MC_BOOT_K\]\s*=\s*\{(.*?)\}", text, flags=re.S).group(1)
    thr = [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]+)ull", body)]
    assert len(thr) == k
    return key, k, thr


BOOT_KEY, BOOT_K, THRESHOLDS = _header_constants()
THR = np.array(THRESHOLDS, dtype=np.uint64)
STAT = {"hits": 0, "cov": 1, "aln": 2}


def mix(z):
    """mc_mix64 (splitmix64's finaliser) on a uint64 array or scalar"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def key(seed, b):
    return mix(mix(U(seed & 0xFFFFFFFFFFFFFFFF) ^ mix(np.asarray(b, dtype=np.uint64))) ^ U(BOOT_KEY))


def weights(seed, b, reads):
    """w(b, r) for replicate(s) b and read ids r (broadcast against each other): the number of thresholds <= u"""
    with np.errstate(over="ignore"):
        u = mix(key(seed, b) + np.asarray(reads, dtype=np.uint64))
    return np.searchsorted(THR, u, side="right").astype(np.int64)


def sums(best, stats, B, seed, replicates=None, threads=1, return_counts=False):
    """mc_bootstrap's outputs for the replicates given (default all of 0 .. B-1): (sums_i64 [len, nfam + 1], sums_f64 [len, nfam]);
    the cov sums as numpy.longdouble accumulations of the float64 terms (64-bit mantissa: the exact sum to within n x 2^-64).
    threads: replicates are independent; numpy releases the GIL in the array operations.  return_counts: also n_f [len, nfam], the
    sum of the weights of every family's hits (its weighted hit count, whatever its aln_stat)."""
    nfam = len(stats)
    st = [STAT.get(s, s) for s in stats]
    reps = list(range(B)) if replicates is None else list(replicates)
    fam = best["family"].astype(np.int64)
    reads = best["read"].astype(np.int64).astype(np.uint64)
    members = [np.nonzero(fam == f)[0] for f in range(nfam)]
    aln = [best["aln"][m].astype(np.int64) for m in members]
    cov = [best["aln"][m].astype(np.float64) / best["target_len"][m].astype(np.float64) for m in members]
    si = np.zeros((len(reps), nfam + 1), np.int64)
    sf = np.zeros((len(reps), nfam), np.float64)
    counts = np.zeros((len(reps), nfam), np.int64)

    def one(j):
        w = weights(seed, reps[j], reads)
        si[j, nfam] = w.sum()
        for f in range(nfam):
            wf = w[members[f]]
            counts[j, f] = wf.sum()
            if st[f] == 0:
                si[j, f] = wf.sum()
            elif st[f] == 2:
                si[j, f] = (wf * aln[f]).sum()
            else:
                terms = wf.astype(np.float64) * cov[f]                    # each term rounded to float64, as the kernel rounds it
                sf[j, f] = np.float64(terms.astype(np.longdouble).sum())
    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(len(reps))))
    else:
        for j in range(len(reps)):
            one(j)
    return (si, sf, counts) if return_counts else (si, sf)


def golden_best(case, families):
    """The best hits of a golden as the device hands them out (BEST_DTYPE, ascending read id).  The golden stores aln and
    aln / target_len; the target length is the integer that reproduces that quotient exactly."""
    from microbecensus_amd import _native
    g = json.load(open(os.path.join(GOLD, case + ".json")))
    idx = {f: i for i, f in enumerate(families)}
    items = sorted(g["best_hits"].items(), key=lambda kv: int(kv[0]))
    arr = np.zeros(len(items), _native.BEST_DTYPE)
    for i, (q, (fam, aln, cov, score)) in enumerate(items):
        tl = int(round(aln / cov))
        assert aln / float(tl) == cov
        arr[i] = (int(q), idx[fam], int(aln), tl, score)
    return arr, g
