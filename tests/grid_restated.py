"""The training workflow's grid classification (training/training.py:229-334: read_hits, aln_filter, pid_filter, score_filter,
find_best_hits, aggregate_hits, classify_reads) restated in plain Python over m8 TEXT, for any grid and any marker set.  Shared by
the CPU test that pins it to the reference's own output and by the GPU tests that use it where no golden exists.

Parsing follows parse_rapsearch (:210-219): pid, the coordinates and the score are floats of the printed fields, aln an int.  The
query coordinates are therefore floats, and the reference's `(query_start_dna + 3 - frame)/3` is a float division even under
Python 2.  All arithmetic is IEEE double, in the reference's order.

One shortcut, stated here because it is the only place the restatement does not walk the reference's loops literally: for a given
(aln_cov, max_pid), find_best_hits over the rows with score >= min_score is the best row over all the rows (the first of the
highest score) if that row's score reaches min_score, and no row otherwise - a cut-off removes only rows scoring below it, and
every row tied with the best survives with it.  So the best row per read is found once per (aln_cov, max_pid), then tested against
every cut-off in the caller's order.  Duplicated and unsorted cut-offs need nothing special."""


def parse_m8(text):
    """[(query, target, pid, aln, qstart, qend, tstart, tend, score)] in file order, typed as parse_rapsearch types them."""
    rows = []
    for line in text.splitlines():
        if not line or line[0] == '#':
            continue
        x = line.split()
        rows.append((x[0], x[1], float(x[2]), int(x[3]), float(x[6]), float(x[7]), float(x[8]), float(x[9]), float(x[11])))
    return rows


def read_hits(rows, gene2fam):
    """read_hits (:229-245): query coordinates to amino-acid space, target coordinates 1-based."""
    hits = []
    for query, target, pid, aln, qstart, qend, tstart, tend, score in rows:
        qs, qe = sorted([qstart, qend])
        frame = qs % 3 if qs % 3 in [1, 2] else 3
        query_start = (qs + 3 - frame) / 3
        query_stop = (qe + 1 - frame) / 3
        ts, te = sorted([tstart + 1, tend + 1])
        hits.append((query, target, gene2fam[target], pid, aln, query_start, query_stop, ts, te, score))
    return hits


def coverage(hit, read_length, gene2len):
    """aln / maxaln of aln_filter (:247-265)."""
    _, target, _, _, aln, query_start, query_stop, target_start, target_stop, _ = hit
    query_len = float(read_length) / 3
    x = min(query_start - 1, target_start - 1)
    z = min(query_len - query_stop, gene2len[target] - target_stop)
    return aln / (x + aln + z)


def classify(m8_text, aln_covs, max_pids, min_scores, gene2len, gene2fam, fams, read_length):
    """The grid of classify_reads (:311-334): {(i_cov, i_pid, i_score, family): (hits, aln, cov)} for every combination and family
    with at least one hit; indexes are positions in the caller's lists, families the names in `fams`."""
    hits = read_hits(parse_m8(m8_text), gene2fam)
    covs = [coverage(h, read_length, gene2len) for h in hits]
    out = {}
    for ic, aln_cov in enumerate(aln_covs):
        aln_ok = [h for h, c in zip(hits, covs) if not c < aln_cov]
        for ip, max_pid in enumerate(max_pids):
            pid_ok = [h for h in aln_ok if not h[3] > max_pid]
            best = {}
            for h in pid_ok:                                   # find_best_hits: the first of the highest score
                if h[0] not in best or best[h[0]][-1] < h[-1]:
                    best[h[0]] = h
            for js, min_score in enumerate(min_scores):
                agg = {}
                for h in best.values():
                    if h[-1] < min_score:
                        continue
                    a = agg.setdefault(h[2], [0, 0, 0.0])
                    a[0] += 1
                    a[1] += h[4]
                    a[2] += float(h[4]) / gene2len[h[1]]
                for fam, (nh, na, nc) in agg.items():
                    assert fam in fams, fam
                    out[(ic, ip, js, fam)] = (nh, na, nc)
    return out


def consequential_ties(m8_text, gene2fam, gene2len):
    """Reads whose highest score is shared by rows that differ in family, alignment length or target length: the reads where
    first-on-tie decides what is counted (over all of a read's rows, before any filter)."""
    rows = parse_m8(m8_text)
    top = {}
    for query, target, pid, aln, qstart, qend, tstart, tend, score in rows:
        t = top.get(query)
        if t is None or t[0] < score:
            top[query] = [score, {(gene2fam[target], aln, gene2len[target])}]
        elif t[0] == score:
            t[1].add((gene2fam[target], aln, gene2len[target]))
    return sum(1 for t in top.values() if len(t[1]) > 1)
