"""Reads of mixed lengths, host side (no GPU): the golden of a mixed-length query file (tests/golden/make_varlen_golden.py, made with
the reference's rapsearch) is reproduced by the oracle, which searches every read on its own - so no read's rows depend on its
neighbours in the file - and scripts/rapsearch_mi355x checks every read's length before it opens a device."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def _golden():
    meta = json.load(open(os.path.join(GOLD, "varlen_reads.json")))
    fasta = gzip.open(os.path.join(GOLD, "varlen_reads.fa.gz"), "rb").read()
    m8 = gzip.open(os.path.join(GOLD, "varlen_reads.m8.gz"), "rb").read()
    return meta, fasta, m8


def test_varlen_golden_is_what_it_says():
    meta, fasta, m8 = _golden()
    assert hashlib.md5(fasta).hexdigest() == meta["reads_md5"] and hashlib.md5(m8).hexdigest() == meta["m8_md5"]
    seqs = fasta.splitlines()[1::2]
    lens = [len(s) for s in seqs]
    assert len(seqs) == meta["reads"] and min(lens) == 12 and max(lens) == 510 and len(set(lens)) == meta["distinct_lengths"]
    assert sum(18 <= x <= 25 for x in lens) == meta["reads_18_25"] > 0 and sum(x < 18 for x in lens) == meta["reads_under_18"] > 0
    assert lens != sorted(lens)
    with_rows = {int(l.split(b"\t")[0]) for l in m8.splitlines()}
    assert len(with_rows) == meta["reads_with_rows"] and min(lens[q] for q in with_rows) >= 18


def test_oracle_reproduces_the_mixed_length_golden(oracle_bin, rapdb_dir, tmp_path):
    meta, fasta, m8 = _golden()
    fa = tmp_path / "varlen.fa"
    fa.write_bytes(fasta)
    out = str(tmp_path / "out.m8")
    subprocess.check_call([oracle_bin, os.path.join(rapdb_dir, "rapdb_2.15"), str(fa), out])
    assert open(out, "rb").read() == m8


def test_rapsearch_executable_refuses_reads_over_510(tmp_path):
    fa = tmp_path / "q.fa"
    fa.write_text(">a\n%s\n>b\n%s\n>c\n%s\n" % ("ACGT" * 30, "A" * 511, "ACG" * 20))
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "rapsearch_mi355x"), "-q", str(fa), "-d", "nodb", "-o", str(tmp_path / "o"),
                        "-t", "n", "-b", "0"], capture_output=True, text=True)
    assert p.returncode == 1 and "query b (record 1) is 511 bases long" in p.stderr


def test_rapsearch_executable_refuses_an_empty_record(tmp_path):
    fa = tmp_path / "q.fa"
    fa.write_text(">a\n%s\n>empty\n>c\n%s\n" % ("ACGT" * 30, "ACG" * 20))
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "rapsearch_mi355x"), "-q", str(fa), "-d", "nodb", "-o", str(tmp_path / "o"),
                        "-t", "n", "-b", "0"], capture_output=True, text=True)
    assert p.returncode == 1 and "query empty (record 1) is 0 bases long" in p.stderr
