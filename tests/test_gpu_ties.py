"""The tie accounting on the device through the C ABI (mc_set_ties; csrc/k_ties.h states the rule) against tests/ties_restated.py applied
to the REFERENCE BINARY's m8 goldens: the example reads on the marker database and the generic database under the three cut-off sets of
test_gpu_abundance.py; independence from ranges and entry points (search at once, in several ranges, search_varlen, search_files with
keep_rows=False); the halving path of a range that overflows its pools; reset, off and on, the refusals; and run_abundance with the
switch end to end.  The counts and the coverage of the same run are held to their own restatements throughout.
(test_ties_host.py asserts that these goldens hold ties: 57 ambiguous reads of up to 6 genes here, 22 in the generic database.)"""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_table_cases as TC
import abundance_restated as R
import coverage_restated as V
import ties_restated as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASE = "config1_example_fq"
CUTS = [dict(), dict(min_ident=60, min_aln=30), dict(min_bits=27.1)]


def _same_counts(got, want):
    return np.array_equal(got["reads"], want["reads"]) and np.array_equal(got["aligned"], want["aligned"]) and got["assigned"] == want["assigned"]


def _same_any(got, want):
    return all(np.array_equal(got[k], want[k]) for k in T.ANY)


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


@pytest.fixture(scope="module")
def golden():
    """the reference binary's m8 of the case restated under the three cut-off sets - computed once, shared, never changed.  The map: the
    first 4,000 genes grouped by their names' prefix (the family), every other gene a group of its own - 20 of the 57 ambiguous reads tie
    inside a group, 37 across two"""
    from microbecensus_amd import _native, abundance
    names, seqs = _native.load_markers()
    lengths = [len(s) for s in seqs]
    gmap = TC.group_map(names)
    group_of, gnames = abundance.group_ids(names, gmap)
    rows = V.rows_from_m8(os.path.join(GOLD, CASE + ".m8.gz"), names)
    return {"rows": rows, "lengths": lengths, "group_of": group_of, "ngroups": len(gnames), "gnames": gnames, "gmap": gmap, "names": names,
            "ties": [T.ties(rows, lengths, group_of, len(gnames), **c) for c in CUTS],
            "cov": [V.coverage(rows, lengths, **c) for c in CUTS], "ab": [R.abundance([r[:6] for r in rows], len(names), **c) for c in CUTS]}


@pytest.mark.parametrize("k", [0, 1, 2], ids=["none", "ident60_aln30", "bits27.1"])
def test_marker_database_equals_the_restatement_of_the_reference_m8(engine, reads, golden, k):
    want, want_ab, want_cov = golden["ties"][k], golden["ab"][k], golden["cov"][k]
    assert want["ambiguous"] >= 7 and max(want["k"]) >= 3 and 0 < want["group_ambiguous"] < want["ambiguous"]     # (ties there are, under every cut-off set, inside groups and across)
    engine.set_abundance(True, **CUTS[k])
    try:
        engine.set_coverage(True)
        engine.set_ties(True, golden["group_of"], golden["ngroups"])
        engine.search(reads)
        got, any_, ab, cov, depth, ms = engine.ties(), engine.ties_coverage(), engine.abundance(), engine.coverage(), engine.coverage_depth(), engine.ties_ms()
    finally:
        engine.set_abundance(False)
    print(CUTS[k], "assigned", ab["assigned"], "ambiguous", got["ambiguous"], "across groups", got["group_ambiguous"], "candidates", int(got["candidates"].sum()),
          "covered", int(cov["covered"].sum()), "covered_any", int(any_["covered_any"].sum()), "ties ms", ms)
    assert ms > 0.0 and ab["searched"] == len(reads) and _same_counts(ab, want_ab)
    assert all(np.array_equal(cov[key], want_cov[key]) for key in ("covered", "spanned", "max_depth")) and np.array_equal(depth, want_cov["depth"])
    assert T.same_counters(got, want) and _same_any(any_, want)
    assert T.invariants(got, ab["reads"], ab["assigned"], golden["group_of"]) == []
    assert (any_["covered_any"] >= cov["covered"]).all() and (any_["max_depth_any"] >= cov["max_depth"]).all()
    if not k:
        assert got["ambiguous"] == 57 and got["group_ambiguous"] == 37 and int(got["candidates"].sum()) == sum(want["k"]) == 194 + 2 * 32 + 3 * 17 + 4 * 4 + 5 * 2 + 6 * 2


def test_generic_database_equals_the_restatement_of_the_reference_m8():
    """18,553 sequences, 20,000 reads, the generic seed path: 22 ambiguous reads, four reads that tie with the same subject twice, 316
    reads whose top score is not in their first row."""
    with I.generic_case() as (eng, names, seqs, rd, meta, m8):
        lengths = [len(s) for s in seqs]
        rows = V.rows_from_m8(m8, names)
        assert len(rows) == meta["m8_rows"]
        group_of = (np.arange(len(names)) // 50).astype(np.int32)
        ngroups = int(group_of.max()) + 1
        for cut in CUTS:
            assert R.cutoffs_clear_of_printed_values(rows, cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
            want, want_ab = T.ties(rows, lengths, group_of, ngroups, **cut), R.abundance([r[:6] for r in rows], len(names), **cut)
            eng.set_abundance(True, **cut)
            eng.set_ties(True, group_of, ngroups)                      # ties first, coverage second: the any-depth comes with the second
            eng.set_coverage(True)
            eng.search(rd)
            got, any_, ab = eng.ties(), eng.ties_coverage(), eng.abundance()
            print(cut, "assigned", ab["assigned"], "ambiguous", got["ambiguous"], "across groups", got["group_ambiguous"], "abundance ms", eng.abundance_ms(),
                  "ties ms", eng.ties_ms(), "of", eng.stats()["ms_total"])
            assert ab["searched"] == len(rd) and _same_counts(ab, want_ab)
            assert T.same_counters(got, want) and _same_any(any_, want)
            assert T.invariants(got, ab["reads"], ab["assigned"], group_of) == []
            if not cut:
                assert got["ambiguous"] == 22


def test_counters_do_not_depend_on_ranges_or_entry_point(engine, reads, golden, tmp_path):
    from microbecensus_amd import _native
    k = 0
    want, want_ab = golden["ties"][k], golden["ab"][k]
    n = len(reads)
    got = {}

    def take(how):
        got[how] = (engine.ties(), engine.ties_coverage(), engine.abundance())

    def zeros():
        t, a, ab = engine.ties(), engine.ties_coverage(), engine.abundance()
        return (not any(t[key].any() for key in T.COUNTERS) and t["ambiguous"] == 0 and t["group_ambiguous"] == 0 and not any(a[key].any() for key in a)
                and ab["searched"] == 0 and ab["assigned"] == 0 and not ab["reads"].any() and not engine.coverage_depth().any())
    engine.set_abundance(True, **CUTS[k])
    try:
        engine.set_coverage(True)
        engine.set_ties(True, golden["group_of"], golden["ngroups"])
        engine.search(reads)
        take("one search")
        engine.abundance_reset()                                           # ... zeroes the tie counters and the any-depth too
        assert zeros() and engine.ties_ms() == 0.0
        between = None
        for lo, hi in ((0, 1000), (1000, 1003), (1003, n)):                # three calls of uneven sizes, no reset in between
            engine.search(reads[lo:hi], first_read_id=lo)
            if hi == 1003:
                between = engine.ties()                                    # a read between two of them changes nothing
        take("three searches, a read in between")
        assert 0 < int(between["candidates"].sum()) < int(want["candidates"].sum())
        engine.abundance_reset()
        engine.upload(reads)
        engine.range_begin(0, 5001, 0)
        engine.range_end()
        engine.range_begin(5001, n - 5001, 5001)
        engine.range_end()
        take("range_begin / range_end")
        engine.abundance_reset()
        engine.search_varlen([bytes(r) for r in reads])
        take("search_varlen")
        engine.abundance_reset()
        fa = tmp_path / "reads.fa"
        fa.write_bytes(gzip.open(os.path.join(GOLD, CASE + ".reads.fa.gz"), "rb").read())
        rd = _native.Reader([str(fa)], 100, 10_000_000, False, 0, -5, -5, 100, False)
        try:
            rows_f, _ = engine.search_files(rd, keep_rows=False)
            assert rd.stats()["sampled"] == n
        finally:
            rd.close()
        assert len(rows_f) == 0 and len(engine.rows()) == 0 and engine.stats()["rows"] == len(golden["rows"])     # no row reached the host; all were made
        take("search_files, keep_rows=False")
        assert engine.ties_ms() > 0.0
    finally:
        engine.set_abundance(False)
    for how, (t, a, ab) in got.items():
        assert ab["searched"] == n and _same_counts(ab, want_ab), how
        assert T.same_counters(t, want) and _same_any(a, want), how


def test_reset_off_and_on(engine, reads, golden, tmp_path):
    want, want_ab, want_cov = golden["ties"][0], golden["ab"][0], golden["cov"][0]
    part = reads[:3000]
    engine.set_abundance(True)
    try:
        engine.set_ties(True)                                              # no map, no coverage
        engine.search(part)
        t = engine.ties()
        assert len(t["group_unique"]) == 0 and t["group_ambiguous"] == 0 and 0 < int(t["candidates"].sum())
        with pytest.raises(RuntimeError, match="coverage is off"):
            engine.ties_coverage()
        engine.set_coverage(True)                                          # coverage second: zeros everywhere, and the any-depth is there
        assert engine.abundance()["searched"] == 0 and not engine.ties()["candidates"].any() and not engine.ties_coverage()["covered_any"].any()
        engine.search(reads)
        t, a = engine.ties(), engine.ties_coverage()
        assert all(np.array_equal(t[key], want[key]) for key in ("candidates", "unique", "share")) and t["ambiguous"] == want["ambiguous"] and _same_any(a, want)
        engine.set_coverage(False)                                         # coverage off: the any-depth goes, the counters stay
        with pytest.raises(RuntimeError, match="coverage is off"):
            engine.ties_coverage()
        assert np.array_equal(engine.ties()["share"], want["share"])
        engine.set_ties(False)                                             # ties off: the counts stay, the path is the one without
        with pytest.raises(RuntimeError, match="ties are off"):
            engine.ties()
        assert engine.ties_ms() == 0.0 and _same_counts(engine.abundance(), want_ab)
        engine.abundance_reset()
        rows_off, _ = engine.search(reads)
        assert _same_counts(engine.abundance(), want_ab)
        engine.set_coverage(True)
        engine.set_ties(True, golden["group_of"], golden["ngroups"])                 # on again, with a map: zeros, of the counts and the depth too
        assert engine.abundance()["searched"] == 0 and not engine.coverage_depth().any() and not engine.ties()["share"].any()
        engine.search(reads)
        assert T.same_counters(engine.ties(), want) and _same_any(engine.ties_coverage(), want) and np.array_equal(engine.coverage_depth(), want_cov["depth"])
        engine.set_abundance(False)                                        # ... turns ties off with it
        with pytest.raises(RuntimeError, match="ties are off"):
            engine.ties()
    finally:
        engine.set_abundance(False)
    g = json.load(open(os.path.join(GOLD, CASE + ".json")))               # the rows of a run beside the counts alone: today's, by the golden's md5
    out = str(tmp_path / "off.m8")
    engine.search(reads)
    engine.write_m8(out)
    assert len(rows_off) == g["m8_rows"] and hashlib.md5(open(out, "rb").read()).hexdigest() == g["m8_md5"]


def test_a_range_that_overflows_its_pools_adds_once(monkeypatch):
    """The recipe and size of test_gpu_abundance.py's test_a_range_that_overflows_its_pools_counts_once: 24,000 marker-dense reads on an
    engine of their own take the halving path (asserted) - also with the rows staying on the device.  The tie counters of the one call
    must be those of 5,000-read batches (which fit: no split) and the restatement's on that run's own host rows."""
    from microbecensus_amd import _native, abundance
    names, seqs = _native.load_markers()
    lengths = [len(s) for s in seqs]
    group_of, gnames = abundance.group_ids(names, {n: n.split("_")[0] for n in names})     # every gene in its family's group
    ngroups = len(gnames)
    cut = I.DENSE_CUT

    def switches(eng):
        eng.set_abundance(True, **cut)
        eng.set_coverage(True)
        eng.set_ties(True, group_of, ngroups)
    runs = I.dense_runs(monkeypatch, switches, lambda eng: (eng.ties(), eng.ties_coverage(), eng.abundance(), eng.abundance_ms(), eng.ties_ms()), stay=True)
    rd, (st, one), (st5, five, rows5), (stay, stay_rows) = runs["reads"], runs["one"], runs["five"], runs["stay"]
    print("one call:", st["range_splits"], "splits,", st["rows"], "rows; abundance ms", one[3], "ties ms", one[4], "of", st["ms_total"])
    assert st["range_splits"] > 0, "the batch did not overflow: the test no longer exercises the halving path"
    assert st5["range_splits"] == 0 and st5["rows"] == st["rows"] == len(rows5)
    assert stay_rows == 0
    one, five, stay = one[:3], five[:3], stay[:3]
    want = T.ties(V.rows_from_array(rows5), lengths, group_of, ngroups, **cut)
    print("restated:", len(want["k"]), "reads,", want["ambiguous"], "ambiguous, largest tied set", max(want["k"]))
    assert len(want["k"]) > 10_000 and want["ambiguous"] > 100
    for how, (t, a, ab) in (("5,000-read batches", five), ("one call", one), ("one call, rows on the device", stay)):
        assert ab["searched"] == len(rd) and ab["assigned"] == len(want["k"]), how
        assert T.same_counters(t, want) and _same_any(a, want), how
        assert T.invariants(t, ab["reads"], ab["assigned"], group_of) == [], how


def test_refusals_through_the_abi(engine, reads):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    nseq = len(engine.names)
    buf = np.zeros(nseq, np.int64)
    good = np.zeros(nseq, np.int32)
    assert lib.mc_set_ties(h, 1, None, 0) != 0 and "abundance counting is off" in err()
    assert lib.mc_ties_read(h, buf.ctypes.data, None, None, None, None, None) != 0 and "ties are off" in err()
    assert lib.mc_ties_coverage_read(h, buf.ctypes.data, None, None) != 0 and "ties are off" in err()
    assert lib.mc_ties_ms(h) == 0.0 and lib.mc_set_ties(h, 0, None, 0) == 0          # off while off: nothing to do
    engine.set_abundance(True)
    try:
        assert lib.mc_set_ties(h, 1, good.ctypes.data, -1) != 0 and "ngroups -1 is negative" in err()
        assert lib.mc_set_ties(h, 1, None, 3) != 0 and "NULL group map" in err()
        bad = good.copy()
        bad[nseq - 1] = 3
        assert lib.mc_set_ties(h, 1, bad.ctypes.data, 3) != 0 and ("group_of[%d] = 3 lies outside 0 .. 2" % (nseq - 1)) in err()
        bad[nseq - 1], bad[7] = 0, -1
        assert lib.mc_set_ties(h, 1, bad.ctypes.data, 3) != 0 and "group_of[7] = -1 lies outside 0 .. 2" in err()
        assert lib.mc_ties_read(h, buf.ctypes.data, None, None, None, None, None) != 0 and "ties are off" in err()      # every refusal left them off
        engine.upload(reads[:2000])
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_ties(h, 1, None, 0) != 0 and "in flight" in err()
        engine.range_end()
        engine.set_ties(True, good, 1)
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_ties(h, 0, None, 0) != 0 and "in flight" in err()
        engine.range_end()
        assert engine.abundance()["searched"] == 2000                        # (set_ties(True) zeroed the first range's counts)
        assert lib.mc_ties_coverage_read(h, buf.ctypes.data, None, None) != 0 and "coverage is off" in err()            # ties on, coverage off
        # every refusal has left the handle usable: only candidates asked for; everything asked for; one group holds every read
        assert lib.mc_ties_read(h, buf.ctypes.data, None, None, None, None, None) == 0
        t, ab = engine.ties(), engine.abundance()
        assert np.array_equal(buf, t["candidates"]) and int(buf.sum()) > 0 and t["group_unique"].tolist() == [ab["assigned"]] and t["group_ambiguous"] == 0
        assert T.invariants(t, ab["reads"], ab["assigned"], good) == []
        engine.set_coverage(True)
        engine.set_coverage(False)
        engine.set_ties(False)
        assert lib.mc_ties_coverage_read(h, buf.ctypes.data, None, None) != 0 and "ties are off" in err()
        engine.set_abundance(False)
        assert lib.mc_set_ties(h, 1, None, 0) != 0 and "abundance counting is off" in err()
    finally:
        engine.set_abundance(False)
    rows_ok, _ = engine.search(reads[:2000])                                 # the handle is what it was
    assert len(rows_ok) > 0


def _header(path):
    return [l[2:].rstrip("\n").split(":\t") for l in open(path) if l.startswith("# ")]


def test_run_abundance_with_ties_end_to_end(golden, tmp_path):
    """run_abundance with the packaged markers as the genes, on the example FASTQ under config1's sample options (-n 10000; 100 bp), under
    --ags (no estimate: the test is about the tables): ties alone, with coverage and min_breadth, and with groups."""
    from microbecensus_amd import _native, abundance
    names, lengths, rows = golden["names"], golden["lengths"], golden["rows"]
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    gmap = golden["gmap"]
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % kv for kv in gmap.items()))
    ids, gnames, want = golden["group_of"], golden["gnames"], golden["ties"][0]
    want_ab, want_cov = golden["ab"][0], golden["cov"][0]
    base = {"seqfiles": [fq], "genes": genes, "nreads": 10000, "device": 0, "ags": 3.0e6}
    grp = dict(base, groups=str(tmp_path / "map.tsv"))
    out = [str(tmp_path / ("genes%d.tsv" % k)) for k in range(5)]
    # without the switch: the files of a run with the switch absent, byte for byte - the gene table, the groups table, the depth file
    abundance.run_abundance(dict(grp, outfile=out[0], coverage=True, min_breadth=0.1, depth_out=out[0] + ".depth"))
    abundance.run_abundance(dict(grp, outfile=out[1], coverage=True, min_breadth=0.1, depth_out=out[1] + ".depth", ties=False))
    for ext in ("", ".groups.tsv", ".depth"):
        assert open(out[0] + ext, "rb").read() == open(out[1] + ext, "rb").read(), ext
    # ties alone
    table, args = abundance.run_abundance(dict(base, outfile=out[3], ties=True))
    assert args["ties_ms"] > 0.0 and "covered_any_aa" not in table and "groups_ties" not in table
    ref, tied = open(out[0]).read().split("\n"), open(out[3]).read().split("\n")
    nh = 11
    assert tied[:nh] == ref[:nh] and tied[nh:nh + 2] == ["# ties:\ton", "# reads_ambiguous:\t57"]
    assert tied[nh + 2] == "gene\tlength_aa\treads\taligned_aa\trpkg\tunique_reads\tcandidate_reads\tshared_reads\trpkg_shared"
    body, body0 = [l.split("\t") for l in tied[nh + 3:-1]], [l.split("\t") for l in ref[nh + 4:-1]]
    assert len(body) == len(names) and [r[:5] for r in body] == [r[:5] for r in body0]   # the existing columns: byte for byte
    assert [int(r[2]) for r in body] == want_ab["reads"].tolist()
    assert [int(r[5]) for r in body] == want["unique"].tolist() and [int(r[6]) for r in body] == want["candidates"].tolist()
    shared = [float(np.float64(v) / 4294967296.0) for v in want["share"]]
    assert [r[7] for r in body] == [repr(v) for v in shared]
    ge = abundance.genome_equivalents(table["sampled_reads"], 100, 3.0e6)
    assert [r[8] for r in body] == [repr(float(v)) for v in abundance.rpkg(np.array(shared), np.array(lengths), ge)]
    assert abs(sum(shared) - want_ab["assigned"]) < 1e-6
    # with coverage, min_breadth and groups
    table, args = abundance.run_abundance(dict(grp, outfile=out[4], ties=True, min_breadth=0.1))
    full = open(out[4]).read().split("\n")
    assert full[:nh + 3] == ref[:nh + 3] and full[nh + 3:nh + 6] == ["# ties:\ton", "# reads_ambiguous:\t57", "# reads_ambiguous_across_groups:\t%d" % want["group_ambiguous"]]
    assert full[nh + 6] == ref[nh + 3] + "\tunique_reads\tcandidate_reads\tshared_reads\trpkg_shared\tcovered_any_aa\tbreadth_any\tdetected_any"
    body, body0 = [l.split("\t") for l in full[nh + 7:-1]], [l.split("\t") for l in ref[nh + 4:-1]]
    assert [r[:10] for r in body] == body0 and [r[10:14] for r in body] == [r[5:9] for r in [l.split("\t") for l in tied[nh + 3:-1]]]
    assert [int(r[14]) for r in body] == want["covered_any"].tolist() and [r[15] for r in body] == [repr(c / n) for c, n in zip(want["covered_any"].tolist(), lengths)]
    det_any = [int(c > 0 and float(v) * 1 >= 0.1 * float(n)) for c, v, n in zip(want["candidates"].tolist(), want["covered_any"].tolist(), lengths)]
    det = [int(r[9]) for r in body]
    assert [int(r[16]) for r in body] == det_any and sum(det_any) > sum(det) > 0 and all(a >= d for a, d in zip(det_any, det))
    assert 0 < want["group_ambiguous"] < 57
    gfull, gref = open(out[4] + ".groups.tsv").read().split("\n"), open(out[0] + ".groups.tsv").read().split("\n")
    assert gfull[nh + 6] == gref[nh + 3] and gfull[nh + 7] == gref[nh + 4] + "\tunique_reads\tshared_reads\trpkg_shared\tgenes_detected_any"
    gbody, gbody0 = [l.split("\t") for l in gfull[nh + 8:-1]], [l.split("\t") for l in gref[nh + 5:-1]]
    assert [r[:5] for r in gbody] == gbody0 and [r[0] for r in gbody] == gnames
    assert [int(r[5]) for r in gbody] == want["group_unique"].tolist()                                 # the restatement's group_unique ...
    member_sum = np.bincount(ids, weights=want["unique"], minlength=len(gnames)).astype(np.int64)
    assert (want["group_unique"] >= member_sum).all() and (want["group_unique"] > member_sum).any()      # ... which is not the sum of the members' unique_reads
    gshare = [sum(int(want["share"][k]) for k in np.flatnonzero(ids == g)) for g in range(len(gnames))]
    assert [r[6] for r in gbody] == [repr(v / 4294967296.0) for v in gshare] and sum(gshare) == want_ab["assigned"] << 32
    assert sum(int(r[8]) for r in gbody) == sum(det_any)
    assert int(np.sum(table["group_unique"])) + table["reads_ambiguous_across_groups"] == want_ab["assigned"]
    hdr = dict(_header(out[4] + ".groups.tsv"))
    assert hdr["ties"] == "on" and hdr["reads_ambiguous"] == "57" and hdr["groups"] == str(tmp_path / "map.tsv")
