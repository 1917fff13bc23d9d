/* mcensus.h - C ABI of libmcensus_hip.so: the MI355X (gfx950) implementation of MicrobeCensus' hot path.
 *
 * The reference has no FFI: its hot path is a subprocess,
 *     rapsearch -q tmp -d rapdb_2.15 -o tmp -z T -e 1 -t n -p f -b 0
 * launched by search_seqs()            (/root/reference/microbe_census/microbe_census.py:369-389),
 * whose tmp.m8 is parsed by parse_rapsearch()/classify_reads()          (microbe_census.py:391-460),
 * and whose database comes from `prerapsearch -d markers.faa -n rapdb_2.15` (training/search_reads.py:57
 * documents the flag set).  Each entry point below names the piece of that interface it replaces.
 * Plain pointers and sizes only; every call returns 0 (or a count) on success and a negative value on
 * error, with the message available from mc_last_error().  There is no CPU fallback: without a HIP device
 * mc_open() fails.
 */
#ifndef MCENSUS_H
#define MCENSUS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mc_handle mc_handle;

/* One row of RAPsearch2's m8 output (the 12 columns parse_rapsearch reads, microbe_census.py:391-398),
 * kept binary: query = read id, subject = marker index. */
typedef struct mc_row {
    int32_t query, subject;
    double ident;
    int32_t alnlen, mismatch, gapopen, qstart, qend, sstart, send;
    double loge, bits;
    int32_t score, nmatch;
} mc_row;

/* best_hits[read] = [family, aln, aln/target_len, score]   (classify_reads, microbe_census.py:450-453) */
typedef struct mc_best_hit {
    int32_t read, family, aln, target_len;
    double bits;
} mc_best_hit;

typedef struct mc_stats {
    int64_t reads, seed_tasks, gap_tasks, hsps, rows, reads_with_rows, classified;
    int64_t bucket_lookups, key_probes;   /* algorithmic traffic of the seed kernel: 8 B and 2 B reads */
    /* HIP event intervals of the six stages.  ms_translate is the translation kernel's own interval wherever it ran: where it was
     * issued ahead (mc_range_end) it shared the device with the ordering and finishing kernels of the range before and took longer
     * than alone.  ms_total is the SUM of the six: it can exceed the wall time of a step, in which stages of two ranges overlap. */
    float ms_translate, ms_seed, ms_eval, ms_gapped, ms_sort, ms_finish, ms_total;
    /* what the seed kernel itself asked its structures (timed form): 9-mer filter words (4 B), wildcard filter lines (32 B),
     * pair filter blocks (16 B), bucket records + key groups searched (32 B + 16 B); seed_tasks postings (4 B) came out */
    int64_t seed_exact_asks, seed_wild_asks, seed_pair_asks, seed_probes;
    /* how often a range overflowed the pools sized for shotgun reads and was run again in smaller pieces (mc_run_range) */
    int64_t range_splits;
} mc_stats;

const char *mc_last_error(void);
int mc_device_count(void);

/* Replaces `prerapsearch -d <fasta> -n <db>` + the DB load of rapsearch (CHashSearch::BuildDHash / Search):
 * builds the reduced-alphabet 6-mer index of the marker proteins on the host and uploads it to `device`.
 * marker_family[i] is the gene family index of marker i (gene_fam.map, microbe_census.py:438). */
mc_handle *mc_open(const char *const *names, const char *const *seqs, int32_t nseq,
                   const int32_t *marker_family, int32_t nfam, int32_t device);
void mc_close(mc_handle *h);
/* mc_open() spends half a second of host time building the index (buckets, suffix keys, filters) - more than the search of the
 * reference's default run of 1 - 2 M reads (scripts/run_microbe_census.py:31: one run_pipeline per process).  With a cache directory
 * set (process-wide; NULL or "": none) the built index is kept there in a file named by a hash of the marker names and sequences
 * and read back by later mc_open() calls; a file that does not match its header, sizes, input hash and checksum is ignored and
 * rebuilt.  The directory should be writable by the user alone (the Python layer uses ~/.cache/microbecensus_amd, mode 0700). */
int mc_set_index_cache(const char *dir);
/* Host only (tests; no GPU): builds the index, writes it to dir, reads it back and compares every array, then checks that a file of
 * other sequences, a damaged and a truncated file are refused.  0 = all of that held. */
int mc_index_cache_check(const char *const *names, const char *const *seqs, int32_t nseq, const char *dir);

/* The same from a database `prerapsearch` already wrote (the reference ships one as data/rapdb_2.15): residues, buckets,
 * posting order and suffix keys are taken from the file, the GPU-side structures derived from them.  All markers start in
 * family 0 of 1; name them with mc_marker_name() and assign the families with mc_set_families() (gene_fam.map), then
 * mc_set_run().  mc_rapdb_verify() needs no GPU: 0 if the file holds exactly the index mc_open() builds from the sequences. */
mc_handle *mc_open_rapdb(const char *rapdb_path, int32_t device);
int32_t mc_marker_count(const mc_handle *h);
const char *mc_marker_name(const mc_handle *h, int32_t i);
int mc_set_families(mc_handle *h, const int32_t *marker_family, int32_t nfam);
int mc_rapdb_verify(const char *rapdb_path, const char *const *names, const char *const *seqs, int32_t nseq);
/* ... and the writer (no GPU): what `prerapsearch -d <fasta> -n <path>` produces, <path> and <path>.info. */
int mc_rapdb_write(const char *const *names, const char *const *seqs, int32_t nseq, const char *path);

/* Host views of the index, for cross-checking against a prerapsearch-built database (tests only). */
int mc_index_view(const mc_handle *h, const uint8_t **res_codes, const uint32_t **offsets, const uint32_t **bucket_starts,
                  const uint32_t **postings, const uint16_t **keys, int64_t *nres, int64_t *npostings,
                  uint32_t *freq_thr, double letter_p[10]);

/* Per-run parameters: trimmed read length (args['read_length']), the -e threshold, and
 * find_opt_pars(pars.map, L) (microbe_census.py:61-72) as arrays indexed by family. aln_stat: 0 hits, 1 cov, 2 aln. */
int mc_set_run(mc_handle *h, int32_t read_len, double loge_thr, const double *min_cov, const double *min_score,
               const int32_t *max_aaid, const int32_t *aln_stat);

/* Replaces search_seqs() + classify_reads(): reads = nreads x read_len bytes (the trimmed sequences that
 * process_seqfile writes, one after another, no separators).  Runs the whole device pipeline.
 * first_read_id is added to the read index to form the query id. */
int mc_search(mc_handle *h, const uint8_t *reads, int64_t nreads, int64_t first_read_id);

/* The same on reads of MIXED lengths, as a FASTA holds them: read i is bases[offsets[i] .. offsets[i + 1]) (offsets: nreads + 1
 * ascending values; the reads lie back to back).  Each read is searched at its own length - translation, seeds, extension and the
 * E-value (RAPsearch2's length adjustment of the query) - exactly as `rapsearch` searches it in a file of reads of many lengths;
 * classification (best hits) uses mc_set_run()'s read_len, the nominal length class_reads.py and alignment_coverage divide by.
 * A read shorter than 18 bases has no frame of more than 5 residues, which RAPsearch2 skips: it has no rows.  The reads are bucketed
 * by length on the device and the fixed-length pipeline runs once per bucket; results as after mc_search() (rows in ascending read
 * id = first_read_id + i, RAPsearch2's order within a read; best hits by read id), and mc_write_m8 / mc_write_m8_named take them.
 * A batch whose reads all have mc_set_run()'s length is mc_search() itself.  Refused: an empty read, a read longer than 510 bases
 * (the message names the read), more than 2^31 - 1 reads. */
int mc_search_varlen(mc_handle *h, const uint8_t *bases, const int64_t *offsets, int64_t nreads, int64_t first_read_id);

/* ---- length classes: an estimate from reads of mixed lengths, each at the largest legal length it reaches (csrc/mc_classes.h states
 * the rule).  mc_set_run_classes() replaces mc_set_run() for the class runs that follow: K ascending class lengths (1 <= K <= 32, each
 * 18 .. 510) and the four parameter arrays as [K][nfam], row k = find_opt_pars(pars.map, class_len[k]).  The handle's single-length
 * state (mc_search, mc_upload, ...) is the top class's; a later mc_set_run() restores the single-length run.
 * mc_search_classes(): rows = nreads rows of stride = class_len[K - 1] bytes, a read's bases and then 0 bytes (a read longer than the
 * stride cut to it).  The rows of a batch are sorted into their classes and trimmed on the device (csrc/k_classes.h) and the
 * fixed-length pipeline runs once per non-empty class: that length's tables, that class's classification parameters and
 * classification length.  Results: mc_result_best_hits() in ascending read id = first_read_id + row index, mc_result_best_classes()
 * parallel to them (the class index of every best hit), mc_result_class_reads() (out[k]: the rows of class k; out[K]: the rows below
 * class_len[0], which are skipped) and mc_result_stats() (totals).  mc_set_best_hits_only() is honoured.  A class run hands out NO m8
 * rows: mc_result_rows() is empty and mc_write_m8() writes nothing.  Results do not depend on how the rows were cut into batches and
 * ranges.  A run whose rows all fall in one class returns the best hits of mc_search() at that length on the cut reads, byte for byte.
 * Refused, with a message naming the value: K outside 1 .. 32, a length outside 18 .. 510 or not ascending, a stride other than
 * class_len[K - 1], a range in flight.  mc_search_files() on a reader of mc_reader_open_classes() is the same run from files; it is
 * refused unless the handle's class list equals the reader's. */
int mc_set_run_classes(mc_handle *h, const int32_t *class_len, int32_t K, double loge_thr, const double *min_cov, const double *min_score,
                       const int32_t *max_aaid, const int32_t *aln_stat);
int mc_search_classes(mc_handle *h, const uint8_t *rows, int64_t nreads, int32_t stride, int64_t first_read_id);
int64_t mc_result_best_classes(mc_handle *h, const uint8_t **cls);
int mc_result_class_reads(mc_handle *h, int64_t *out /* [K + 1] */);
/* NOT part of the supported interface (like mc_debug_stage): a test and timing aid that may change or go.  The device prologue alone (row lengths, classes, scan, stable scatter, trimming gather) on nreads <= 2,097,151
 * host rows under the class list of mc_set_run_classes().  Copied out where the pointer is not NULL: perm[nreads] (the row of every
 * sorted position; rows without a class last), start[K + 2] (first sorted position of every class, of the rows without one, and
 * nreads), word0[K + 1] (class k's reads lie back to back at pitch class_len[k] from byte 16 x word0[k] of the sorted bytes), the
 * sorted bytes themselves when they fit sorted_cap, ms[2] (HIP events: [0] lengths, classes, scan and scatter, [1] the gather).
 * Returns the number of sorted bytes, 16 x word0[K], or < 0. */
int64_t mc_debug_classes_prologue(mc_handle *h, const uint8_t *rows, int64_t nreads, int32_t stride, uint32_t *perm, uint32_t *start, int64_t *word0,
                                  uint8_t *sorted, int64_t sorted_cap, float *ms);

/* Same pipeline on reads that are already resident in HBM (bench / streaming):
 * mc_upload() copies a batch to the device, mc_run() executes the kernels on it (no host transfers of reads). */
int mc_upload(mc_handle *h, const uint8_t *reads, int64_t nreads);
/* ... or adopts caller-owned device memory (e.g. a torch uint8 tensor) as the resident read set. */
int mc_attach(mc_handle *h, const void *device_reads, int64_t nreads);
int mc_run(mc_handle *h, int64_t first_read_id);
/* runs the pipeline on reads [first, first+count) of the resident set (count <= 2097151). */
int mc_run_range(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id);

/* A stream of ranges without the device waiting for the host.  mc_range_begin() enqueues the FRONT of a range (translation,
 * seeds, seed evaluation: two thirds of its time) and returns at once; mc_range_end() completes it - results as after
 * mc_run_range(), valid until the next mc_range_end() / mc_run_range().  The order end(i), begin(i + 1), <look at the results
 * of i>, end(i + 1), ... lets the host collect rows and best hits while the device works on the next front (what the host still
 * reads of range i lies in pinned host memory; the pools on the device are free for range i + 1).  One range at a time is on the
 * device: a second mc_range_begin() before mc_range_end() is refused.  mc_search() / mc_search_files() run their batches this
 * way, bench.py its steps.  mc_range_end() returns -2 when the range overflowed a pool: it is then no longer in flight - give
 * it to mc_run_range(), which runs it in smaller pieces.  mc_run_range() and mc_search*() refuse to run while a range is in
 * flight.  Results never depend on any of this.
 * Looking ahead: the translation of the NEXT range needs nothing of this one, and it needs the vector ALUs where the seed search and
 * the seed evaluation wait for memory.  mc_range_begin() therefore issues, on a stream of its own and into the second of two frame
 * buffers, the translation of the range it expects next, which runs beside the front of its own range: the one that follows
 * contiguously in the same resident read set - first + count, up to
 * count reads, clipped to the set, nothing at its end - which is how bench.py and a caller's own stream of ranges walk a set.
 * (mc_search(), mc_search_files() and the calls on reads of mixed lengths know their next range only when the running one ends:
 * theirs is issued by that end, behind the gapped stage, beside the ordering and finishing kernels.)  An
 * mc_range_begin() / mc_run_range() of that range, or of fewer reads from the same first read, with the same resident reads, read
 * length and tables, finds its frames there and starts with the seed kernel; any other range waits for the lookahead's kernel and
 * translates itself.  A wrong guess costs one translation beside work the device was waiting through anyway and never changes a
 * result; whatever replaces reads, tables or pools, mc_debug_stage() and mc_close() wait for a lookahead and discard it.
 * mc_run_range() issues none.  mc_ranges_translated_ahead(): the ranges begun since mc_open() that used a lookahead.
 * mc_stats.ms_translate is a figure of the range's own stream: its own translation (all of it, or the reads behind a lookahead's) plus
 * the time its stream waited for a lookahead's kernel to end, so that the six ms_* stages add up to ms_total.  mc_ahead_kernel_ms():
 * the interval of the lookahead's kernel that the range which ended last used, between its own two events, in the background of the
 * range before it - 0 where the range used none (tools/ahead_trace.py). */
int mc_range_begin(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id);
int mc_range_end(mc_handle *h);
int mc_ranges_in_flight(const mc_handle *h);
int64_t mc_ranges_translated_ahead(const mc_handle *h);
float mc_ahead_kernel_ms(const mc_handle *h);

/* Test aid (tests/test_gpu_parity.py, per-stage parity with the CPU emulation of the kernels' per-thread code): what the stages of
 * the last mc_run_range() left on the device - what = 0: the six translated, SEG-masked frames of every read (rows of
 * *record_bytes bytes; BuildQHash@0x40b530, Seg::*), 1: the seed hits (16-byte records; Searching@0x415050), 2: the gap tasks
 * (28 bytes; ExtendSeq2Set@0x413b90), 3: the HSP pool (48 bytes; CalRes@0x4077a0), 4: the counts of the gapped extension's chain
 * of kernels (tests/test_gpu_gapped_chain.py), three uint32 - the distinct flanks it extended, those it sent to the second, wider
 * window, those it sent on to full-size rows (AlignGapped@0x40a550); defined for a range that ran unsplit (mc_stats.range_splits
 * == 0), 5: one uint32, the form of k_translate_seg the last range launched - 1: the block's reads staged in LDS, 0: read from global
 * memory (tests/test_gpu_translate_seg.py), 6: one uint32, its instantiation - 1: narrow (frames of at most 63 residues, reads up to
 * 191 bp), 0: wide (tests/test_gpu_translate_seg_narrow.py).  Returns the number of bytes (copied to dst when they fit cap_bytes; dst may be NULL to ask for the size), -1 on error. */
int64_t mc_debug_stage(mc_handle *h, int what, void *dst, int64_t cap_bytes, int32_t *record_bytes);
/* Test aid (tests/test_gpu_owned.py): what the library holds of the HIP runtime in this process, over all handles - out[0] device
 * buffers, [1] pinned host buffers, [2] streams, [3] events.  Counted where each is made and destroyed (csrc/mc_owned.h). */
void mc_debug_live(int64_t out[4]);

/* The seed kernel can count the index reads of the reference's algorithm for the batch (mc_stats.bucket_lookups /
 * key_probes: what CHashSearch::Searching@0x415050 / ExtendSeq2Set@0x413b90 would read - bench.py reports the rate at which
 * the timed kernel disposes of them).  Off by default: the two fields stay 0 and the kernel answers most one-substitution
 * probes from its wildcard and pair filters instead of searching them (mc_stats.seed_* count what it asks).  With on != 0
 * every probe is searched and counted.  Results do not depend on it. */
int mc_set_counting(mc_handle *h, int on);

/* Results of the last mc_search()/mc_run(), owned by the handle until the next call:
 * rows in the reference's m8 order (ascending read id, then RAPsearch2's order within a read); best hits in
 * ascending read id (only reads with a passing hit). */
int64_t mc_result_rows(mc_handle *h, const mc_row **rows);
int64_t mc_result_best_hits(mc_handle *h, const mc_best_hit **hits);
int mc_result_stats(mc_handle *h, mc_stats *out);

/* Writes the rows of the last run as RAPsearch2 m8 text (PrintRes formatting: %g columns, tab separated,
 * no header lines) - what search_seqs() leaves in paths['tempfile']+'.m8'. append != 0 appends. */
int mc_write_m8(mc_handle *h, const char *path, int append);
/* The same with the Query column taken from query_names[query id - first_read_id] (rapsearch prints the FASTA header's first
 * token; process_seqfile names its reads 0, 1, ... so the two agree there) - for the rapsearch-compatible executable. */
int mc_write_m8_named(mc_handle *h, const char *path, int append, const char *const *query_names, int64_t n_names, int64_t first_read_id);

/* The training workflow's grid search (training/training.py:311-334 classify_reads, called by training/class_reads.py:51-66 with
 * 4 aln_covs x 6 max_pids x 27 min_scores) over the m8 rows of the last mc_search() / mc_run(): for every combination, the rows
 * that pass alignment coverage >= aln_cov, identity <= max_pid (integers, as in class_reads.py), bit score >= min_score; per
 * read the best-scoring survivor (the first on a tie); per family the number of such reads, the sum of their alignment lengths,
 * the sum of alignment length / target length.  Outputs are [n_cov][n_pid][n_score][nfam] arrays; hits and aln are exact, the
 * coverage sums are accumulated in no fixed order (1e-12 relative against the reference's sequential sum).  One device pass.
 * Cut-offs may come in any order and repeat.  Refused: more than 8 aln_covs, 8 max_pids or 64 min_scores, and a NaN or infinite
 * aln_cov or min_score. */
int mc_grid_classify(mc_handle *h, const double *aln_covs, int32_t n_cov, const int32_t *max_pids, int32_t n_pid, const double *min_scores, int32_t n_score,
                     int64_t *count_hits, int64_t *count_aln, double *count_cov);

/* The uncertainty of an AGS estimate: the per-family sums of aggregate_hits (microbe_census.py:462-472) under B Poisson-bootstrap
 * replicates of the sample, in one device pass.  Replicate b gives the read of best hit i the weight w(b, best[i].read) - Poisson(1),
 * a pure function of (seed, b, read id): csrc/mc_boot.h states the formula and holds its threshold table - so the result does not
 * depend on how the sample was split into batches, ranges or GPUs, nor on the order of best[].  best: n best hits as
 * mc_result_best_hits() hands them out (of one run, of several gathered, or classified from a foreign m8).  family_stat[f]: the
 * family's aln_stat as mc_set_run() numbers it (0 hits, 1 cov, 2 aln).  Outputs, zeroed first:
 *   sums_i64 [B][nfam + 1]   hits family: sum of w; aln family: sum of w x aln; cov family: 0; column nfam: sum of w over all best
 *                            hits (the classified reads the replicate drew).  Exact, whatever the launch geometry.
 *   sums_f64 [B][nfam]       cov family: sum of w x (aln / target_len); others 0.  Each term rounded once, added in an order that
 *                            depends on (n, B) alone: within (terms - 1) x 2^-53 of the exact sum, the same on every run.
 * Refused: nfam outside 1 .. 32, B outside 1 .. 65536, a best hit whose family lies outside 0 .. nfam - 1, whose read id or alignment
 * length is negative or whose target length is < 1.  Needs mc_open() only (no mc_set_run()). */
int mc_bootstrap(mc_handle *h, const mc_best_hit *best, int64_t n, const int32_t *family_stat, int32_t nfam, int32_t B, uint64_t seed,
                 int64_t *sums_i64, double *sums_f64);
/* Milliseconds the last mc_bootstrap()'s kernels took (HIP events; the upload of the hits and the download of the sums not included). */
float mc_bootstrap_ms(const mc_handle *h);

/* Training step 5 (TRAINING.txt; the reference's optimize_weights.R): the per-family weights of one read length, fitted by the
 * deterministic candidate search csrc/mc_wfit.h states - every generation C weight vectors around the best so far, made on the device
 * from a hash of (seed, read_len, generation, candidate, family), each scored by mue = the median over the libraries of
 * |truth - weighted mean of the kept predictions| / truth.  pred[N][F]: the predictions of training_preds.map, NaN for "NA";
 * truth[N]: the true sizes.  Which predictions a library keeps is _ags_of_sums' cut (|pred - median| < 1.48 x MAD), made once.
 * C = 0 and G = -1 select the header's defaults; G = 0 returns the start.  Outputs:
 *   weights [F]          the fitted weights, each in [0, 1]; 1 / F for a family no library keeps
 *   trace   [G + 1][3]   per generation: the best mue so far, the index of the generation's winning candidate (0: nothing was
 *                        better; -1: the search had ended, sigma < 2^-20), sigma after it.  Row 0 is the start: mue(1 / F), 0, sigma.
 * The result is the statement's bit for bit, whatever the launch geometry: the same bytes on every run.
 * Refused: F outside 1 .. 32, N outside 1 .. 4096, C outside 0 .. 65536, G outside -1 .. 4096, a truth that is not a positive finite
 * number, an infinite prediction.  Needs mc_open() only. */
int mc_fit_weights(mc_handle *h, const double *pred, const double *truth, int32_t N, int32_t F, uint64_t seed, int32_t read_len, int32_t C, int32_t G,
                   double *weights, double *trace);
/* mue of K weight vectors of the caller's, w[K][F] -> out[K]: the mask and the kernel arithmetic of mc_fit_weights (+inf where
 * more than half of the libraries keep no family of positive weight).  Refused as mc_fit_weights refuses, and a weight outside
 * [0, 1] or NaN, K outside 0 .. 16777216.  Needs mc_open() only. */
int mc_weights_mue(mc_handle *h, const double *pred, const double *truth, int32_t N, int32_t F, const double *w, int32_t K, double *out);
/* Milliseconds the kernels of the last mc_fit_weights() / mc_weights_mue() took (HIP events; the table's upload and the results'
 * download not included). */
float mc_fit_weights_ms(const mc_handle *h);

/* ---- training (the reference's training/ workflow, TRAINING.txt steps 1 - 3, on the device) --------------------------------
 * A genome resident in HBM: bases = contig_off[ncontig] bytes, the contigs one after another as the FASTA holds them (line breaks
 * dropped, case kept); contig_off[0] = 0.  mc_simulate() writes reads [first, first + n) of library (seed, library_id) at
 * read_len to dst_host (n x read_len bytes): error-free single-end reads of training/seq_sim.py, uniform over every (contig,
 * start) with start + read_len <= contig length, forward strand; each read a pure function of (seed, library_id, read index) -
 * csrc/k_simulate.h states the formula.  A genome without a contig of read_len bases is refused. */
typedef struct mc_genome mc_genome;
mc_genome *mc_genome_open(const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, int32_t device);
void mc_genome_close(mc_genome *g);
int mc_simulate(mc_genome *g, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host);
/* The kind of library mc_simulate() and mc_train_library() make of this genome from now on (training/seq_sim.py -e, -r, -p, -i):
 * error_model MC_ERR_NONE, MC_ERR_UNIFORM (error_rate per consumed base, in [0, 1]) or MC_ERR_ILLUMINA (position-dependent rate of
 * sim_functions.py); paired_end with insert >= the read length: row 2k is mate 1 of fragment k (forward), row 2k + 1 mate 2 (the
 * reverse complement of the fragment's last read_len bases).  Every read keeps read_len bases: the first read_len the error
 * process emits (the reference's reads are read_len + insertions - deletions long: mc_genome_set_read_lengths below gives those).
 * csrc/mc_simlib.h states the formula.  NULL
 * restores the default (single end, no errors).  Refused: an unknown model, a rate outside [0, 1], paired end with insert < 1 or
 * longer than every contig; at simulation time, insert < read_len and (mc_train_library) an odd number of paired-end reads. */
enum { MC_ERR_NONE = 0, MC_ERR_UNIFORM = 1, MC_ERR_ILLUMINA = 2 };
typedef struct mc_library { int32_t paired_end, insert, error_model; double error_rate; } mc_library;
int mc_genome_set_library(mc_genome *g, const mc_library *lib);
/* The read lengths of the libraries mc_simulate_varlen() and mc_train_library() make of this genome from now on.  MC_READLEN_FIXED
 * (default): every read keeps read_len bases, as above.  MC_READLEN_REFERENCE: seq_sim.py's reads - the walk consumes the fragment
 * bases 0 .. read_len - 1 and emits what the error process makes of them, read_len + insertions - deletions bases (the same draws;
 * under MC_ERR_NONE the two modes give the same reads); csrc/mc_simlib.h states the formula.  A read of more than 510 bases is refused
 * when it is simulated (the message names it), never cut.  Refused: any other mode. */
enum { MC_READLEN_FIXED = 0, MC_READLEN_REFERENCE = 1 };
int mc_genome_set_read_lengths(mc_genome *g, int32_t mode);
/* Reads [first, first + n) of library (seed, library_id) in the reference read-length mode (whatever the genome's mode): their bases
 * back to back into dst_host (range by range while they fit in dst_cap bytes; dst_host NULL: none - call so to learn the size) and
 * offsets[0 .. n] (offsets[0] = 0; always written).  Returns the total number of bases, or < 0. */
int64_t mc_simulate_varlen(mc_genome *g, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host,
                           int64_t dst_cap, int64_t *offsets);
/* One library pass: reads [0, nreads) of library (seed, library_id) at mc_set_run()'s read length and E-value threshold, simulated
 * straight into the handle's resident read buffer range by range (MC_STREAM_BATCH reads; mc_upload's buffer: the resident read set
 * is the last range afterwards), searched, and grid-classified on the device as mc_grid_classify() does it (same arguments and
 * outputs).  No m8 row leaves the device; only the grid's bins come back.  The genome must lie on the handle's device.  The
 * last run's rows and best hits are empty afterwards; mc_result_stats() holds the search's totals. */
int mc_train_library(mc_handle *h, mc_genome *g, int64_t nreads, uint64_t seed, uint64_t library_id, const double *aln_covs, int32_t n_cov,
                     const int32_t *max_pids, int32_t n_pid, const double *min_scores, int32_t n_score, int64_t *count_hits, int64_t *count_aln, double *count_cov);
/* In the reference read-length mode a range is simulated in two passes, bucketed by length on the device, and every bucket is searched
 * at its own length (mc_search_varlen) and grid-classified into the same bins - classification at mc_set_run()'s read length, as
 * class_reads.py passes it.  The bases of the last mc_train_library()'s reads: nreads x read_len in the fixed mode, their real
 * total in the reference mode (the reference's rate denominator, training.py's library_sizes). */
int64_t mc_train_library_bases(const mc_handle *h);
/* Milliseconds of the last mc_train_library() from HIP events: [0] simulation (and, in the reference mode, bucketing), [1] search (the stages' own events), [2] grid. */
int mc_train_times(const mc_handle *h, float *ms);

/* ---- mock communities: how good is a model on a metagenome of known composition --------------------------------------------
 * A community resident in HBM: M member genomes with copies[m] cells each (1 <= M <= 65,536; 1 <= copies <= 2^20).  bases and
 * contig_off as for mc_genome_open(), the contigs of all members one after another; member m holds contigs
 * member_first_contig[m] .. member_first_contig[m + 1] - 1 (member_first_contig[0] = 0, [M] = ncontig; every member has a contig).
 * A community library is what shotgun sequencing of the mixture gives: a read comes from member m with probability proportional
 * to copies[m] x (valid starts of m), and inside the member it is mc_simulate()'s read - csrc/mc_simlib.h states the draw.  A
 * read is a pure function of (seed, library_id, read index); both mates of a fragment come from one member; a community of one
 * member with one copy gives mc_simulate()'s library of that genome, byte for byte, for every library kind. */
typedef struct mc_community mc_community;
mc_community *mc_community_open(const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, const int32_t *member_first_contig,
                                const int64_t *copies, int32_t M, int32_t device);
void mc_community_close(mc_community *c);
/* The kind of library the community's calls make from now on: the kinds and refusals of mc_genome_set_library() (paired end: an
 * insert longer than every contig of every member is refused).  NULL restores the default.  Reads always keep read_len bases
 * (MC_READLEN_FIXED): a community has no reference read-length mode. */
int mc_community_set_library(mc_community *c, const mc_library *lib);
/* Reads [first, first + n) of library (seed, library_id) at read_len to dst_host (n x read_len bytes), as mc_simulate().  A member
 * without a contig of the span (read_len, or the insert) is never drawn.  Refused: a community none of whose members has such a
 * contig, one whose universe (the sum of copies x valid starts) reaches 2^62, insert < read_len. */
int mc_community_simulate(mc_community *c, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host);
/* One library pass, fused: reads [0, nreads) of library (seed, library_id) at mc_set_run()'s read length and settings, simulated
 * straight into the handle's resident read buffer range by range (MC_STREAM_BATCH reads, global read ids) and searched from there.
 * Afterwards mc_result_best_hits() / mc_result_stats() are those of mc_search() on the same reads with best hits only
 * (mc_set_best_hits_only); mc_result_rows() is empty.  No read and no m8 row leaves the device.  The community must lie on the
 * handle's device; a paired-end library has an even number of reads; at most 2^31 - 1 reads. */
int mc_community_library(mc_handle *h, mc_community *c, int64_t nreads, uint64_t seed, uint64_t library_id);
/* out[m], m < M: the reads of the last mc_community_simulate() / mc_community_library() that came from member m (counted on the
 * device while they were made; a mate counts as a read). */
int mc_community_member_reads(mc_community *c, int64_t *out);
/* Milliseconds of the last mc_community_library() from HIP events: [0] simulation, [1] search (the stages' own events). */
int mc_community_times(const mc_handle *h, float *ms);

/* ---- host stage in front of the search: native read sampler (csrc/mc_reader.cpp; no GPU involved) ----------------
 * Replaces open_file / parse_seqs / quality_filter / process_seqfile (microbe_census.py:47-59, :294-325, :265-279,
 * :328-367) and count_bases (:573-584) with identical results, quirks included (see the header of mc_reader.cpp).
 * Plain, .gz and .bz2 inputs (libbz2 is bound at run time).  Errors: NULL / negative + mc_reader_last_error(); -3 = the
 * reference would have raised inside run_pipeline (its message names the Python exception). */
typedef struct mc_reader mc_reader;
typedef struct mc_reader_stats {
    int64_t sampled, too_short, low_qual, dups;   /* the four counts process_seqfile prints (:362-366) */
    int64_t records;                              /* records parsed before the sampler stopped */
    int64_t bases;                                /* their total sequence length ... */
    int64_t exhausted;                            /* ... which is count_bases() (:573-584) when every file was read to its end (1) */
    int64_t ragged_end;                           /* the data ended inside a FASTQ record (a truncated file; a byte window that does not end on a record boundary) */
} mc_reader_stats;

const char *mc_reader_last_error(void);
/* Caps the worker threads of the host stages (record parsing, parallel inflate) of every reader opened afterwards: the reference's
 * args['threads'] (-t, microbe_census.py:270, forwarded there to rapsearch -z).  n <= 0: the CPUs the process may use (cgroup quota), up to 32 (default). */
void mc_set_host_threads(int32_t n);
/* fastq: args['file_type'] == 'fastq'; quality_offset: 32 or 64 as auto_detect_quality_offset returns it (:175-187);
 * fasta_out (may be NULL): the temp FASTA process_seqfile writes, ">{id}\n{seq[:L]}\n" per accepted read. */
mc_reader *mc_reader_open(const char *const *paths, int32_t npaths, int32_t read_len, int64_t nreads, int32_t fastq, int32_t quality_offset,
                          double min_quality, double mean_quality, double max_unknown, int32_t filter_dups, const char *fasta_out);
/* The same head-take under length classes (csrc/mc_classes.h): a record's L is its class length class_len[k], the largest one it
 * reaches.  Too short: below class_len[0]; the N share and the quality mean and minimum run over the first L bases and qualities; the
 * duplicate test on the full sequence, as ever; sampling stops at nreads accepted reads in all.  An accepted read is one row of
 * mc_reader_stride() = class_len[K - 1] bytes - its first L bases, then 0 bytes - and the temp FASTA holds seq[:L].  mc_reader_stats is
 * unchanged (the per-class counts come from the search: mc_result_class_reads).  mc_reader_run / _reads / _start / _fetch / _join and
 * mc_search_files() work on such a reader; the window, part and slice readers below have no class form.  Refused as
 * mc_set_run_classes() refuses a class list. */
mc_reader *mc_reader_open_classes(const char *const *paths, int32_t npaths, const int32_t *class_len, int32_t K, int64_t nreads, int32_t fastq,
                                  int32_t quality_offset, double min_quality, double mean_quality, double max_unknown, int32_t filter_dups, const char *fasta_out);
/* bytes per row of mc_reader_reads() / mc_reader_fetch(): the read length, or the top class length */
int32_t mc_reader_stride(const mc_reader *r);
/* The same sampler on the byte window [byte_lo, byte_hi) of ONE plain (uncompressed, regular) file: the records that start in it.
 * Both ends are moved to the first record start behind them by one rule ('@' line whose second next line starts with '+' in a file
 * that starts with '@'; '>' line in one that starts with '>'), so consecutive windows cut a file into whole records whoever reads
 * them: the ranks of a multi-GPU run sample their own slices side by side (microbecensus_amd/distributed.py) and reproduce the
 * head-take of process_seqfile (:337-356) from the per-slice counts.  No duplicate filter (it needs the whole stream in one place). */
mc_reader *mc_reader_open_range(const char *path, int64_t byte_lo, int64_t byte_hi, int32_t read_len, int64_t nreads, int32_t fastq,
                                int32_t quality_offset, double min_quality, double mean_quality, double max_unknown);
/* -d (filter_dups) with a sampler on every rank.  The duplicate rule of process_seqfile (:345 the test comes before the quality filter,
 * :354 only accepted reads enter the set) is class-local: a record's fate depends on nothing but the earlier records with the same
 * sequence or its reverse complement.  So parsing, quality filter and hashing run on every rank's own byte window
 * (mc_reader_open_range + mc_reader_describe: one 32-byte descriptor per record), the ranks exchange the descriptors, every rank gives
 * every record of the round its verdict with mc_dupset_walk (same input, same verdicts; sequences are compared on the file's own
 * mapping) and copies the accepted reads of its own window with mc_reader_take (microbecensus_amd/distributed.py).
 * flags / verdict bits: 1 too short, 2 has qualities, 4 a base outside ACGTN, 8 accepted, 16 fails the quality filter, 32 duplicate,
 * 64 the reference raises at this record. */
typedef struct mc_rec_desc { uint64_t h1, h2; uint64_t seq_off; uint32_t len; uint8_t flags, pad[3]; } mc_rec_desc;
typedef struct mc_dupset mc_dupset;
int64_t mc_reader_describe(mc_reader *r, const mc_rec_desc **out);   /* records of the window (array owned by the reader), or < 0; mc_reader_stats.ragged_end: not usable, fall back */
mc_dupset *mc_dupset_open(void);
void mc_dupset_close(mc_dupset *s);
int mc_dupset_walk(mc_dupset *s, const char *path, const mc_rec_desc *d, int64_t n, uint8_t *verdict);   /* n descriptors of `path` in file order -> n verdicts; the set remembers across calls and files */
int64_t mc_reader_take(mc_reader *r, const uint8_t *verdict, int64_t n, int64_t max_take, uint8_t *dst);   /* accepted reads of the described window (first read_len bases), at most max_take */
/* The same sampler on the blocks [block_lo, block_hi) of ONE .bz2 file (open_file :55-58): the records that start in the TEXT of those
 * blocks, both ends moved to the first record start behind them by the rule of mc_reader_open_range.  The blocks of a bzip2 file are
 * independent (csrc/mc_pbzip2.h), so the ranks of a multi-GPU run decode and sample their own shares side by side - which a .gz does not
 * allow.  kind: '@' or '>' (what a record of the file starts with).  mc_bz2_blocks(): the number of blocks of a file all of whose streams
 * check out from its first to its last byte, or -1 (cut short, damaged, trailing bytes: one sampler reads such a file and reports what the
 * reference would).  No duplicate filter. */
mc_reader *mc_reader_open_bz2_part(const char *path, int64_t block_lo, int64_t block_hi, int32_t kind, int32_t read_len, int64_t nreads, int32_t fastq,
                                   int32_t quality_offset, double min_quality, double mean_quality, double max_unknown);
int64_t mc_bz2_blocks(const char *path);
/* A .gz file across the ranks.  A gzip member cannot be entered in the middle (every block may point 32 KB back) but it can be DECODED
 * from the middle speculatively (csrc/mc_pgzip.h): the file is cut into slices of chunks, every rank decodes its slice at once, and what
 * is sequential is a chain of hand-overs - where the slice in front ended and the 32 KB in front of that - after which every rank samples
 * the records that start in its slice's text (both ends moved to the first record start behind them, as mc_reader_open_range).
 *   mc_gz_chunks            chunks of chunk_bytes the parallel reader cuts the file into, or -1 (not a gzip file it takes)
 *   mc_reader_open_gz_part  the sampler on chunks [chunk_lo, chunk_hi); run it with mc_reader_start / mc_reader_join (it waits for the state)
 *   mc_reader_gz_provide    what mc_reader_gz_end_state of the slice in front returned (n = 0: that slice failed); not needed for chunk_lo = 0
 *   mc_reader_gz_end_state  waits until the slice is stitched; returns the bytes written (at most 32784), or -1
 *   mc_reader_gz_finish     after mc_reader_join: checks the CRCs of the members that end in the slice, given CRC (4 bytes) | length (8 bytes) of
 *                           the open member's bytes in front of it (zeros for the first slice); 0, or -3 = gzip.open's "CRC check failed" */
int64_t mc_gz_chunks(const char *path, int64_t chunk_bytes);
mc_reader *mc_reader_open_gz_part(const char *path, int64_t chunk_lo, int64_t chunk_hi, int64_t chunk_bytes, int32_t kind, int32_t read_len, int64_t nreads,
                                  int32_t fastq, int32_t quality_offset, double min_quality, double mean_quality, double max_unknown);
int mc_reader_gz_provide(mc_reader *r, const uint8_t *state, int64_t n);
int64_t mc_reader_gz_end_state(mc_reader *r, uint8_t *out, int64_t cap);
int mc_reader_gz_finish(mc_reader *r, const uint8_t *crc_in, uint8_t *crc_out);
/* Runs the sampler: returns args['sampled_reads'] (0 = "No reads remaining after filtering"). */
int64_t mc_reader_run(mc_reader *r);
/* sampled x read_len bytes, row i = trimmed read i: exactly what mc_search() / mc_upload() take. Owned by the reader. */
const uint8_t *mc_reader_reads(mc_reader *r);
int mc_reader_get_stats(mc_reader *r, mc_reader_stats *out);
/* Seconds of the last mc_reader_run() by phase, up to n values (returns how many were written): [0] the whole run; on the sampler's own
 * thread: [1] waiting for input (inflate), [2] guessing the pieces' starts, [3] the parse (all workers), [4] stitching the pieces,
 * [5] verdicts, places and copies of the accepted reads, [6] of [5]: the walkers of the duplicate classes (-d; process_seqfile :345, :354). */
int32_t mc_reader_times(const mc_reader *r, double *out, int32_t n);
void mc_reader_close(mc_reader *r);
/* A closed reader leaves its read buffer (touched pages) to the next reader of the process: the second run_pipeline() of a process pays
 * neither munmap nor page faults.  At most keep_bytes of it are kept (default 4 GB); mc_reader_trim() sets the limit and releases
 * what is held beyond it (0: everything). */
void mc_reader_trim(int64_t keep_bytes);
/* count_bases(): total sequence length over every record of every file. */
int64_t mc_count_bases(const char *const *paths, int32_t npaths);
/* auto_detect_quality_offset() (microbe_census.py:175-187): 32 or 64 by the first quality character of the file that decides
 * (32 when none does); -2 = a record without a quality line (take the Python path: it fails the way the reference does). */
int32_t mc_quality_offset(const char *path);

/* Streaming form of the sampler: mc_reader_start() runs it on a thread of its own; mc_reader_fetch() blocks until reads
 * [first, first + max_reads) are sampled (or the sampler has ended), copies them to dst and returns how many there were
 * (0: no more; negative: the sampler's error); mc_reader_join() waits for the end and returns what mc_reader_run() would have. */
int mc_reader_start(mc_reader *r);
int64_t mc_reader_fetch(mc_reader *r, int64_t first, int64_t max_reads, uint8_t *dst);
int64_t mc_reader_join(mc_reader *r);
int32_t mc_reader_read_len(const mc_reader *r);
/* the nreads the reader was opened with: how many reads it delivers at most (mc_search_files sizes its buffers by it) */
int64_t mc_reader_nreads(const mc_reader *r);

/* process_seqfile() + search_seqs() + classify_reads() in one call (microbe_census.py:328-460): the sampler runs beside the
 * search, batches of accepted reads go through pinned staging memory to the GPU while the batch before is searched.  Results as
 * after mc_search(); the reader's statistics (mc_reader_get_stats) are complete when it returns.  -3: the reference would have
 * raised while sampling (mc_last_error names the Python exception). */
int mc_search_files(mc_handle *h, mc_reader *r, int64_t first_read_id);
/* The same over n_dev GPUs of this process (the multi-device entry; the one-process-per-GPU form with an RCCL
 * reduce is microbecensus_amd/distributed.py): handles[d] was opened on device d and given the same mc_set_run(); the sampler
 * runs once, batches of accepted reads are dealt to the devices as they ask for them (global read ids), one host thread per
 * device.  Results stay with the handles (mc_result_* per handle): the caller adds the per-family sums - integers. */
int mc_search_files_multi(mc_handle *const *handles, int32_t n_dev, mc_reader *r, int64_t first_read_id);
/* keep != 0 (default): mc_search() / mc_search_files() collect the m8 rows of all their batches for mc_result_rows(); 0: only the
 * best hits and the statistics (the rows are still computed - classification reads them on the device). */
int mc_set_keep_rows(mc_handle *h, int keep);
/* on != 0: the runs that follow produce the best hits only (what classify_reads :432-460 keeps) - no m8 rows.  A read none of
 * whose HSPs would pass its family's thresholds (min_cov, max_aaid, min_score) as an m8 row cannot be classified, whatever its
 * ranking: only the reads that have such an HSP are sorted and finished (with ALL their HSPs: ranking, sum statistics and the
 * 500-row cap are the reference's).  mc_result_best_hits() is identical to the full path's; mc_result_rows() is empty and
 * mc_stats.rows / reads_with_rows count the finished reads only.  run_pipeline() uses it when it is not asked for the
 * "reads hit marker proteins" line (verbose). */
int mc_set_best_hits_only(mc_handle *h, int on);

/* ---- gene abundances: the numerator of RPKG ------------------------------------------------------------------------------------
 * The reference's README gives the use of genome equivalents in its section "Normalization":
 *     RPKG = (reads mapped to gene) / (gene length in kb) / (genome equivalents).
 * The reference leaves "reads mapped to gene" to a search of the user's own; the engine is that search (any protein FASTA of up to
 * 32,767 sequences of up to 2,047 residues), and these calls count its result per subject on the device, so that no m8 row has to
 * reach the host.  csrc/k_abundance.h states the rule: a row passes when 100 x nmatch >= min_ident x alnlen, alnlen >= min_aln,
 * bits >= min_bits and loge <= max_loge; a read's best row is the passing row of the highest bit score, the first on a tie
 * (classify_reads' `best < score`, microbe_census.py:450); it adds 1 to reads[subject], alnlen to aligned[subject] and 1 to assigned.
 * searched counts the reads of every range that completed.  All counters are 64-bit integers: exact, whatever the batches, ranges
 * and launch geometry.
 * mc_set_abundance(on != 0) zeroes the counters and sets the cut-offs; from then on every range that completes - mc_search,
 * mc_search_varlen, mc_run / mc_run_range, mc_range_begin + mc_range_end, mc_search_files - adds to them until they are reset.  A
 * range that overflowed a pool (mc_range_end's -2) adds nothing: the pieces mc_run_range runs it in do, each once.  With
 * mc_set_keep_rows(h, 0) the rows of such a run stay on the device: mc_result_rows() is empty and nothing but the best hits is copied
 * to the host.  on == 0 frees the counters and restores the path without them exactly.
 * Refused, with a message naming the value: min_ident outside 0 .. 100, a negative min_aln, a NaN cut-off, a range in flight, best
 * hits only switched on (the counts need every row of a read; mc_set_best_hits_only(h, 1) is refused in turn while they are on).
 * While they are on, mc_search_classes, mc_search_files on a reader of length classes, mc_train_library and mc_community_library are
 * refused (the first two not under mc_set_abundance_classes, below).  mc_search_files_multi keeps one table per handle: the caller adds them (integers). */
int mc_set_abundance(mc_handle *h, int on, int32_t min_ident, int32_t min_aln, double min_bits, double max_loge);
/* Zeroes the counters and mc_abundance_ms() (README "Normalization": one sample, one table).  Refused while the counts are off. */
int mc_abundance_reset(mc_handle *h);
/* The numerators of the README's "Normalization" formula as they stand: reads[s] and aligned[s] per subject s (arrays of
 * mc_marker_count() values; either may be NULL), the reads searched and the reads assigned.  Refused while the counts are off. */
int mc_abundance_read(mc_handle *h, int64_t *reads /* [nseq] */, int64_t *aligned /* [nseq] */, int64_t *searched, int64_t *assigned);
/* Milliseconds the counting kernels took since the last reset (HIP events; one kernel per completed range) - the device cost of the
 * README's "reads mapped to gene" beside mc_stats.ms_total of the same ranges. */
float mc_abundance_ms(const mc_handle *h);

/* ---- coverage breadth and depth of the genes, beside the counts -----------------------------------------------------------------
 * A high RPKG (README "Normalization") may be a few hundred reads piled on one conserved domain; whether the gene is there shows in
 * the fraction of its residues that a read covers.  csrc/k_coverage.h states the rule: the subject span of a row is the residues
 * sstart .. send, 0-BASED AND INCLUSIVE (mc_row.sstart / send; columns 9 and 10 of RAPsearch2's m8); a read's best row - the very row
 * that mc_set_abundance counts - adds 1 to the depth of each of them.  Per subject: covered = residues of depth > 0, spanned = the sum
 * of the depths = the sum of send - sstart + 1 over the best rows, max_depth = the largest depth.  Exact integers, whatever the
 * batches, ranges and launch geometry; the depth is 32-bit (2^32 reads on one residue wrap), spanned 64-bit.
 * mc_set_coverage(on != 0) allocates and zeroes the depth's difference array (residues + subjects 32-bit slots) and ALSO zeroes the
 * abundance counters of the README's "Normalization" numerators: counts and depth describe the same reads.  From then on every
 * range that adds to the counts marks its best rows' spans, in the same kernel; a range that overflowed a pool marks nothing, its
 * pieces once.  on == 0 frees the array and restores the path without it exactly.  mc_set_abundance(h, 0, ...) also turns coverage
 * off; mc_abundance_reset() also zeroes the depth and mc_coverage_ms().
 * Refused, with a message naming the cause: abundance counting off (README "Normalization": mc_set_abundance first), a range in flight.
 * mc_search_files_multi keeps one array per handle: DEPTH adds across handles (mc_coverage_depth, spanned), covered and max_depth do
 * not - the caller recomputes them from the summed depth. */
int mc_set_coverage(mc_handle *h, int on);
/* covered[s], spanned[s] and max_depth[s] per subject s as they stand (arrays of mc_marker_count() values; any may be NULL) - the
 * breadth and depth that qualify the README's "Normalization" numerators: one scan kernel per call.  Refused while coverage is off. */
int mc_coverage_read(mc_handle *h, int64_t *covered /* [nseq] */, int64_t *spanned /* [nseq] */, int64_t *max_depth /* [nseq] */);
/* The depth of every residue, the subjects one after the other in FASTA order (no sentinels): the per-residue picture behind the
 * README's "Normalization" counts.  n must equal the database's residue total (the sum of the sequence lengths); otherwise, and
 * while coverage is off, refused - with both numbers in the message. */
int mc_coverage_depth(mc_handle *h, uint32_t *depth /* [n] */, int64_t n);
/* Milliseconds the scan kernels of mc_coverage_read / mc_coverage_depth took since the last reset (HIP events).  The marks ride in
 * the counting kernel: their time is part of mc_abundance_ms() (README "Normalization": the device cost of "reads mapped to gene"). */
float mc_coverage_ms(const mc_handle *h);

/* ---- the genes that tie for a read's best hit, beside the counts ------------------------------------------------------------------
 * "Reads mapped to gene" (README "Normalization") gives a read to the FIRST row of the highest bit score, and among near-identical
 * sequences - alleles, variants, families - most reads tie: the first of them gets every count, its siblings none.  csrc/k_ties.h
 * states the rule: T is the highest bit score among a read's passing rows; the read's tied set is the DISTINCT subjects that have a
 * passing row with bits == T (exact double equality; any row order; a subject that ties twice is in it once), k its size.  A read
 * that mc_set_abundance does not assign adds nothing.  Per subject: candidates = reads whose tied set holds it, unique = reads whose
 * tied set is it alone, share = in units of 2^-32, floor(2^32 / k) per read to every tied subject and the remainder to the first
 * tied one - the subject the read is assigned to - so that the shares sum to assigned x 2^32.  Scalars: ambiguous = reads with
 * k > 1; with a group map, group_ambiguous = reads whose tied set spans two groups and group_unique[g] = reads whose whole tied set
 * lies in group g.  With coverage on, the first tied row of EVERY tied subject marks its span in a second depth (the "any" depth).
 * All are 64-bit integers: exact, whatever the batches, ranges and launch geometry.
 * mc_set_ties(on != 0) takes the map group_of[nseq] with values in 0 .. ngroups - 1 (or NULL and 0: no groups), and zeroes the tie
 * counters AND the abundance counters and depth of the README's "Normalization" numerators: all describe the same reads.  From then
 * on every range that adds to the counts runs one more kernel behind the counting kernel, on the same rows where they lie (also with
 * mc_set_keep_rows(h, 0)); a range that overflowed a pool adds nothing, its pieces once.  The any-depth exists exactly while ties and
 * coverage are both on, whichever was set second.  on == 0 frees everything and restores the path without it exactly.
 * mc_set_abundance(h, 0, ...) also turns ties off; mc_abundance_reset() also zeroes the tie counters, the any-depth and mc_ties_ms().
 * Refused, with a message naming the cause: abundance counting off (README "Normalization": mc_set_abundance first), a range in flight,
 * a group_of entry outside 0 .. ngroups - 1, ngroups < 0, ngroups > 0 with a NULL map.
 * mc_search_files_multi keeps one set of counters per handle: every counter adds across handles; covered_any and max_depth_any do not. */
int mc_set_ties(mc_handle *h, int on, const int32_t *group_of /* [nseq] or NULL */, int32_t ngroups);
/* The tie counters as they stand, beside the README's "Normalization" numerators of mc_abundance_read: per subject candidates, unique
 * and share (arrays of mc_marker_count() values), group_unique per group (zero values without a map), and the two scalars
 * (group_ambiguous is 0 without a map).  Any pointer may be NULL.  Refused while ties are off. */
int mc_ties_read(mc_handle *h, int64_t *candidates /* [nseq] */, int64_t *unique /* [nseq] */, uint64_t *share /* [nseq] */, int64_t *group_unique /* [ngroups] */,
                 int64_t *ambiguous, int64_t *group_ambiguous);
/* covered_any[s], spanned_any[s] and max_depth_any[s] per subject s: mc_coverage_read's figures of the any-depth - the breadth a gene
 * of the README's "Normalization" table would have if every tied read were its own.  Any pointer may be NULL; one scan kernel per call
 * (its time is part of mc_coverage_ms()).  Refused while coverage or ties is off. */
int mc_ties_coverage_read(mc_handle *h, int64_t *covered_any /* [nseq] */, int64_t *spanned_any /* [nseq] */, int64_t *max_depth_any /* [nseq] */);
/* Milliseconds the tie kernels took since the last reset (HIP events; one kernel per completed range) - beside mc_abundance_ms(), the
 * device cost of the README's "reads mapped to gene". */
float mc_ties_ms(const mc_handle *h);

/* ---- a rarefaction curve beside the counts: the gene table's figures at K nested prefixes of the sample ---------------------------
 * Was the sample sequenced deeply enough, or would twice the reads have found more genes?  csrc/k_curve.h states the rule: with K
 * points n_0 <= ... <= n_{K-1} (64-bit, each >= 1, repeats allowed; 1 <= K <= 64) a read with a best row - the one mc_set_abundance
 * counts - and global id q (first_read_id plus its index) falls into bin b(q) = the number of k with n_k <= q and adds 1 and its
 * alignment length to that bin of its subject; with coverage on it also lowers the "first id" of every residue of its span to
 * min(first, q).  At read time point k is, per subject: reads and aligned summed over the bins 0 .. k, covered = the residues whose
 * first id is below n_k - exactly what mc_abundance_read and mc_coverage_read return after a run on the first n_k reads alone.
 * All are 64-bit integers: exact, whatever the batches, ranges and launch geometry; a range that overflowed a pool adds nothing, its
 * pieces once.
 * mc_set_curve(h, K, points) copies the points and zeroes the curve AND the abundance counters, depth and ties: all describe the
 * same reads; K == 0 frees everything and restores the path without it exactly.  From then on every range that adds to the counts
 * runs one more kernel behind the counting kernel (and the tie kernel), on the same rows where they lie.  mc_set_abundance(h, 0, ...)
 * also turns the curve off; mc_abundance_reset() also zeroes it and mc_curve_ms(); mc_set_coverage in either direction keeps the
 * curve on (going on zeroes everything, as always).
 * Refused, with a message naming the value: K < 0 or K > 64, a point < 1 or below the one before it, abundance counting off, a range
 * in flight.  While the curve is on mc_search_varlen is refused: its rows carry the sorted position, not the caller's read id. */
int mc_set_curve(mc_handle *h, int32_t K, const int64_t *points /* [K] */);
/* The curve as it stands: reads, aligned and covered are K x nseq values, point k of subject s at [k * nseq + s]; assigned: K values,
 * the reads assigned among the first n_k; beyond: the assigned reads with an id >= n_{K-1} - they are in no point.  Any pointer may
 * be NULL; one scan kernel per call.  Refused while the curve is off, and when covered is asked for with coverage off. */
int mc_curve_read(mc_handle *h, int64_t *reads /* [K * nseq] */, int64_t *aligned /* [K * nseq] */, int64_t *covered /* [K * nseq] or NULL */, int64_t *assigned /* [K] */,
                  int64_t *beyond);
/* The number of points the curve is on with - the K that sizes mc_curve_read's arrays; 0 while it is off. */
int32_t mc_curve_k(const mc_handle *h);
/* Milliseconds the curve's kernels took since the last reset (HIP events): one kernel per completed range plus one scan per
 * mc_curve_read. */
float mc_curve_ms(const mc_handle *h);

/* ---- the bootstrap of the counts: how sure an RPKG is ------------------------------------------------------------------------------
 * csrc/mc_geneboot.h states the rule.  While it is on every read with a best row - the one mc_set_abundance counts - also appends
 * (global read id, subject), 8 bytes, to a device list of `capacity` entries: one more kernel behind the counting kernel (and the tie and
 * curve kernels) of every range, on the same rows where they lie.  A read that does not fit adds 1 to `dropped` and writes nothing.
 * mc_set_gene_bootstrap(h, capacity) makes the list and zeroes it AND the abundance counters, depth, ties and curve: all describe the
 * same reads; capacity == 0 frees everything and restores the path without it exactly.  mc_set_abundance(h, 0, ...) also turns it off;
 * mc_abundance_reset() also empties the list and zeroes mc_gene_bootstrap_ms().
 * Refused, with a message naming the value: capacity < 0 or > 2^31 - 1, abundance counting off, a range in flight.  While it is on
 * mc_search_varlen is refused: its rows carry the sorted position, not the caller's read id. */
int mc_set_gene_bootstrap(mc_handle *h, int64_t capacity);
/* B Poisson-bootstrap replicates (1 <= B <= 4096) of the counts as they stand: replicate b weighs read q by
 * mc_boot_weight(mc_boot_key(seed, b), q) - the weights of mc_bootstrap, so replicate b of both is the same resample of the same
 * reads.  counts (or NULL): the replicate counts c[b][s] at [s * B + b], exact integers.  scale: B doubles; replicate b is used when
 * scale[b] is finite and > 0, its value is (double)c[b][s] * scale[b].  stats: six doubles per subject at [6 * s]: the sum of the used
 * values, the sum of their squared distances from their mean, and the sorted used values at floor((m - 1) * 0.025), the next,
 * floor((m - 1) * 0.975), the next (m the number of used replicates; the next index is clamped to m - 1); all NaN with m == 0.  The sums
 * are added in the order csrc/mc_geneboot.h writes down: the same bits on every run.  dropped (or NULL): the reads that did not fit
 * the list; when it is not zero the call returns an error that names the number and computes nothing.  The list is only read: ranges
 * may go on counting after a call. */
int mc_gene_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale /* [B] */, int64_t *counts /* [nseq * B] or NULL */, double *stats /* [nseq * 6] */,
                      int64_t *dropped);
/* Milliseconds the gene bootstrap's kernels took since the last reset (HIP events): one kernel per completed range plus three per
 * mc_gene_bootstrap. */
float mc_gene_bootstrap_ms(const mc_handle *h);
/* The bootstrap of a table of GROUPS of genes (csrc/mc_groupboot.h states the rule) on the same replicates: group_of[s] in
 * 0 .. ngroups - 1 is the group of gene s, gene_kb[s] a finite double > 0, the gene's length in kb.  A group's replicate count is the sum
 * of its members' replicate counts; its replicate value, of a used b, is the sum over its members, in ascending gene index, of
 * (double)c[b][s] * scale[b] / gene_kb[s].  counts (or NULL): the group replicate counts at [G * B + b]; stats: per group the six
 * doubles mc_gene_bootstrap gives per gene, of the group's used replicate values (a group without reads: zeros; no used replicate:
 * NaN).  The sums are added in the order the header writes down: the same bits on every run.  The replicate counts of the genes stay on
 * the device: they are those a preceding mc_gene_bootstrap left there when that call had the same B and seed and no range has
 * completed since, and made here otherwise - either way the same bits.  dropped: as mc_gene_bootstrap's.
 * Refused, with a message naming the value: the gene bootstrap off, B outside 1 .. 4096, a NULL array, ngroups outside 1 .. the genes,
 * a group_of entry outside 0 .. ngroups - 1, a gene_kb entry that is not finite and > 0, a range in flight, dropped != 0. */
int mc_group_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale /* [B] */,
                       const int32_t *group_of /* [nseq] */, int32_t ngroups, const double *gene_kb /* [nseq] */,
                       int64_t *counts /* [ngroups * B] or NULL */, double *stats /* [ngroups * 6] */, int64_t *dropped);
/* Milliseconds the kernels of the mc_group_bootstrap calls took since the last reset (HIP events): two per call, and three more where
 * the call had to make the genes' replicate counts. */
float mc_group_bootstrap_ms(const mc_handle *h);
/* Of those, the milliseconds of k_groupboot_values and of k_groupboot_summary (either pointer may be NULL). */
void mc_group_bootstrap_kernels_ms(const mc_handle *h, float *values_ms, float *summary_ms);

/* ---- the bootstrap of the tie shares: how sure an rpkg_shared is ---------------------------------------------------------------------
 * csrc/mc_tieboot.h states the rule.  It extends mc_set_gene_bootstrap from the counts to the shares of mc_set_ties: while it is on every
 * read that mc_set_ties counts also appends one entry per subject of its tied set - (global read id, subject, share - 1), 12 bytes; a
 * share is the floor(2^32 / k), plus the remainder for the first tied subject, that mc_ties_read adds to share[] - to a device list of
 * `capacity` entries: one more kernel behind the gene bootstrap's of every range, on the same rows where they lie.  An entry that does
 * not fit adds 1 to `dropped` and writes nothing.  mc_set_tie_bootstrap(h, capacity) makes the list and zeroes it AND every abundance
 * counter, as the other switches do; capacity == 0 frees everything and restores the path without it exactly.  mc_set_ties and
 * mc_set_gene_bootstrap - off, or set anew - also turn it off: set it behind them.  mc_abundance_reset() also empties the list and zeroes
 * mc_tie_bootstrap_ms().
 * Refused, with a message naming the value: capacity < 0 or > 2^27 (no replicate sum can wrap below that), ties off, the gene bootstrap
 * off, a range in flight.  While it is on mc_search_varlen is refused, as under mc_set_gene_bootstrap. */
int mc_set_tie_bootstrap(mc_handle *h, int64_t capacity);
/* mc_gene_bootstrap's contract on the shares (it extends it: the same B, seed, scale, weights and six doubles): shares (or NULL): the
 * replicate shares cs[b][s] at [s * B + b], exact integers in units of 2^-32 - the sum over the reads whose tied set holds s of
 * weight x share.  Replicate b is used when scale[b] * 2^-32 is finite and > 0, its value is (double)cs[b][s] * (scale[b] * 2^-32).
 * For every b the shares add up to 2^32 times mc_gene_bootstrap's counts.  stats, dropped: as mc_gene_bootstrap's, dropped counting
 * entries; when it is not zero the call returns an error that names the number and computes nothing. */
int mc_tie_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale /* [B] */, uint64_t *shares /* [nseq * B] or NULL */, double *stats /* [nseq * 6] */,
                     int64_t *dropped);
/* Milliseconds the tie bootstrap's kernels took since the last reset (HIP events), as mc_gene_bootstrap_ms: one kernel per completed
 * range plus three per mc_tie_bootstrap. */
float mc_tie_bootstrap_ms(const mc_handle *h);
/* Of those, the milliseconds of k_tieboot_collect and of the reads' kernels (as mc_group_bootstrap_kernels_ms; either pointer may be NULL). */
void mc_tie_bootstrap_kernels_ms(const mc_handle *h, float *collect_ms, float *read_ms);

/* ---- the bootstrap of the coverage columns: how much a breadth and a detection call hang on single reads ----------------------------
 * csrc/mc_covboot.h states the rule.  While it is on every read that mc_set_abundance assigns also appends one entry - (global read id,
 * subject, sstart, send of its best row), 12 bytes; a span that mc_set_coverage keeps out of the depth is stored as the empty span - to a
 * device list of `capacity` entries: one more kernel behind the other bootstraps' of every range, on the same rows where they lie (behind
 * the gene fold: in gene space).  An entry that does not fit adds 1 to `dropped` and writes nothing.  mc_set_coverage_bootstrap(h,
 * capacity) makes the list and zeroes it AND every abundance counter, as the other switches do; capacity == 0 frees everything and restores
 * the path without it exactly.  mc_set_abundance(off) and mc_set_coverage(off) also turn it off: set it behind them.  It needs neither
 * mc_set_gene_bootstrap nor mc_set_ties.  mc_abundance_reset() also empties the list and zeroes mc_coverage_bootstrap_ms().
 * Refused, with a message naming the value: capacity < 0 or > 2^31 - 1, the counts off, coverage off, a range in flight.  While it is on
 * mc_search_varlen is refused, as under mc_set_gene_bootstrap. */
int mc_set_coverage_bootstrap(mc_handle *h, int64_t capacity);
/* B replicates (1 .. 4096) of the covered residues as they stand, under mc_bootstrap's weights: read q is present in replicate b when its
 * weight under (seed, b) is > 0, and covered[s * B + b] (or NULL) is the number of residues of gene s that the best rows of its present
 * reads cover - at most mc_coverage_read's covered[s], since a Poisson(1) resample leaves out about 37 % of the reads.  stats: the six
 * doubles of mc_gene_bootstrap (sum, m2, x[lo], x[lo + 1], x[hi], x[hi + 1]) of those B values, in residues, every replicate used; zeros
 * for a gene without reads.  need (or NULL): nseq values >= 1; detected (or NULL, only with need): detected[s] is the number of
 * replicates with covered >= need[s].  dropped: the assigned reads that did not fit the list; when it is not zero the call returns an
 * error that names the number and computes nothing.  Refused too: B outside 1 .. 4096, a need of 0, detected without need, the switch
 * off, a range in flight. */
int mc_coverage_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const uint32_t *need /* [nseq] or NULL */, int64_t *covered /* [nseq * B] or NULL */,
                          double *stats /* [nseq * 6] */, int64_t *detected /* [nseq] or NULL */, int64_t *dropped);
/* Milliseconds the coverage bootstrap's kernels took since the last reset (HIP events), as mc_gene_bootstrap_ms: one kernel per
 * completed range plus three per mc_coverage_bootstrap. */
float mc_coverage_bootstrap_ms(const mc_handle *h);
/* Of those, the milliseconds of k_covboot_collect and of the reads' kernels (either pointer may be NULL). */
void mc_coverage_bootstrap_kernels_ms(const mc_handle *h, float *collect_ms, float *read_ms);

/* ---- the counts on class runs: gene abundances from reads of mixed lengths -------------------------------------------------------
 * README "Reads of mixed lengths": a class run searches every read at the largest length class it reaches.  With this switch on the
 * abundance counts ride on such a run: mc_search_classes and mc_search_files on a reader of length classes are no longer refused
 * while the counts are on; every piece of every class makes its rows, leaves them on the device and adds to the counts, the depth and
 * the ties as a fixed-length range does (same kernels), and the best hits of the class run are returned as without the counts.
 * `searched` grows by every row of every batch, the rows below the lowest class included.  The gene bootstrap takes the GLOBAL id of
 * a read - first_read_id plus its row in the call - through a map that the class prologue leaves on the device: replicate b is the
 * same resample whatever the classes, batches and pieces.  Ids stay below 2^31.
 * A per-class table (csrc/k_abund_classes.h) holds, per class, the rows sorted into it and the reads of it assigned to a gene, and
 * the rows below the lowest class: the n_k of a mixed-length denominator, sum n_k x L_k bases.  It is summed on the device, zeroed
 * with the counts by every switch that zeroes them and by mc_abundance_reset(), and freed when the switch or the counts go off.
 * mc_set_abundance_classes(on != 0) zeroes every counter; on == 0 restores the refusal and the path without it exactly.
 * Refused, with a message naming the value: abundance counting off, a range in flight, the curve on (mc_set_curve is refused in turn
 * while the switch is on: a prefix of reads of mixed lengths has no one length).  mc_search_varlen stays as it is. */
int mc_set_abundance_classes(mc_handle *h, int on);
/* The per-class table as it stands: rows[k] and assigned[k] of class k = 0 .. n - 2 of mc_set_run_classes, and at n - 1 the rows
 * below the lowest class (assigned 0).  Either pointer may be NULL.  Refused while the switch is off and when n is not the number of
 * classes + 1 - with both numbers in the message. */
int mc_abundance_classes_read(mc_handle *h, int64_t *rows /* [n] */, int64_t *assigned /* [n] */, int32_t n);
/* Milliseconds the per-class table's kernel took since the last reset (HIP events; one single-thread kernel per piece). */
float mc_abundance_classes_ms(const mc_handle *h);

/* ---- Genes longer than one database sequence: segments and the fold (csrc/mc_fold.h states the rule) ------------------------------
 * The engine opens no sequence of more than 1,192 residues (MC_FOLD_SEG_LEN).  A longer gene is searched as overlapping segments -
 * segment j at offset j x (MC_FOLD_SEG_LEN - MC_FOLD_OVERLAP), consecutive ones sharing MC_FOLD_OVERLAP = 512 residues - each an ordinary
 * sequence of the index, and a kernel (csrc/k_fold.h) folds every row of a finished range back onto its gene before any abundance
 * kernel sees it: subject -> the gene's index, sstart and send shifted by the segment's offset.  The caller cuts the genes (the Python
 * layer: abundance.split_genes) and says how with three maps.
 * mc_open_stats() is mc_open() with the totals of the UNSPLIT database: stat_nseq sequences of stat_nres residues enter the length
 * adjustment and the search space of every table, so bits and loge of an alignment are those it has against the unsplit genes.
 * Nothing else reads them; refused: stat_nseq < 1 or stat_nres < stat_nseq.
 * mc_set_gene_fold(): seg_gene[s] and seg_off[s], the gene and the offset in it of sequence s of the index; gene_len[g], the residues of
 * gene g; ngenes == 0 turns the fold off.  While it is on every size of the abundance ABI above - the arrays of mc_abundance_read,
 * mc_coverage_read, mc_coverage_depth, mc_depth_stats, mc_ties_read (and group_of), mc_ties_coverage_read, mc_curve_read and mc_gene_bootstrap - is
 * the GENES': mc_abundance_count() sequences, mc_abundance_residues() residues (the index's while it is off).  Rows handed to the host
 * (mc_result_rows, m8) stay what the engine produced.  Set it BEFORE mc_set_abundance: with the counts on it is refused unless the
 * tables keep their sizes, and then it zeroes every counter like the other switches.
 * Refused, with a message naming the value: a range in flight; a map that does not ascend gene by gene from gene 0 to ngenes - 1;
 * offsets that are not j steps of one step S into their gene; an inner segment that does not have the one length L > S or does not
 * end before its gene does; a last segment that does not end where gene_len says; a gene of more than 65,535 residues; coverage
 * offsets (the sum of gene_len + 1) that pass 2^32.
 * mc_gene_fold_stats(): ngenes (0: off); edge_rows, the rows since the last zeroing whose span touched an interior segment edge
 * (sstart == 0 on a segment that is not its gene's first, or send on the last residue of one that is not its gene's last) - the
 * witness that the overlap was wide enough, not a filter; ms, the fold kernel's milliseconds since then (HIP events).  Any may be NULL. */
mc_handle *mc_open_stats(const char *const *names, const char *const *seqs, int32_t nseq, const int32_t *marker_family, int32_t nfam, int32_t device,
                         int64_t stat_nres, int32_t stat_nseq);
int mc_set_gene_fold(mc_handle *h, int32_t ngenes, const int32_t *seg_gene /* [nseq] */, const int32_t *seg_off /* [nseq] */, const int32_t *gene_len /* [ngenes] */);
int mc_gene_fold_stats(mc_handle *h, int32_t *ngenes, int64_t *edge_rows, float *ms);
int32_t mc_abundance_count(const mc_handle *h);
int64_t mc_abundance_residues(const mc_handle *h);

/* ---- How similar the assigned reads are to the database's sequence, beside the counts (csrc/mc_identity.h states the rule) ----------
 * "Reads mapped to gene" (README "Normalization") says how many reads a gene got, not how close they are to it: at 99 % identity they
 * are that allele, at 65 % a distant homolog.  A read's best row - the very row that mc_set_abundance counts, under the same
 * 0 <= subject < nseq - adds 1 to hist[subject][bin], bin = alnlen < 1 ? 0 : (100 * nmatch) / alnlen in integer division (the floor of
 * the identity in percent, 0 .. 100: 101 bins of 32 bits), and nmatch, mismatch and gapopen to three 64-bit sums of the subject.  Exact
 * integers, whatever the batches, ranges, classes and launch geometry.
 * mc_set_identity(on != 0) allocates the histogram (128 counters per sequence: 101 bins, padded) and the sums, and zeroes them AND every
 * other abundance counter: all describe the same reads.  From then on every range that adds to the counts adds to them, in a kernel of
 * its own behind the others (csrc/k_identity.h), pieces of class runs included; under a gene fold in gene space.  on == 0 frees them and
 * restores the path without it exactly.  mc_set_abundance(h, 0, ...) also turns the identity off; mc_abundance_reset() also zeroes it and
 * both times below.
 * Refused, with a message naming the value: abundance counting off (mc_set_abundance first), a range in flight. */
int mc_set_identity(mc_handle *h, int on);
/* The identity as it stands, per sequence s (arrays of mc_abundance_count() values; any may be NULL): the three sums; ident_min and
 * ident_max, the lowest and highest non-empty bin; ident_median, the LOWER median - the smallest bin whose cumulative count reaches
 * (n - 1) / 2 + 1, n the reads of s; ge[s * nlevels + j], the reads of s in bins >= levels[j].  A sequence without reads gets -1 for the
 * three bins and 0 elsewhere.  One scan kernel per call, a wave per sequence: the histogram stays on the device.
 * Refused, naming the value: the identity off; nlevels outside 0 .. 8; a level outside 0 .. 100 or not above the one before it. */
int mc_identity_read(mc_handle *h, const int32_t *levels /* [nlevels] */, int32_t nlevels, int64_t *matched /* [nseq] */, int64_t *mismatched /* [nseq] */,
                     int64_t *gap_opens /* [nseq] */, int32_t *ident_min /* [nseq] */, int32_t *ident_median /* [nseq] */, int32_t *ident_max /* [nseq] */,
                     int64_t *ge /* [nseq * nlevels] or NULL */);
/* The histogram itself, without its padding: hist[s * 101 + bin].  Refused while the identity is off, and a NULL array. */
int mc_identity_hist(mc_handle *h, uint32_t *hist /* [nseq * 101] */);
/* Milliseconds since the last reset (HIP events): of the counting side's kernel over the completed ranges, and of the scan kernels of
 * mc_identity_read. */
float mc_identity_ms(const mc_handle *h);
float mc_identity_scan_ms(const mc_handle *h);

/* ---- Is the gene there, and how many copies?  Order statistics of a gene's depth (csrc/mc_depthstats.h states the rule) ----------------
 * "Reads mapped to gene" (README "Normalization") and mean_depth both rise when a few hundred reads pile on one conserved domain; an order
 * statistic of the per-residue depth does not.  With d the depth of mc_set_coverage, sorted to x[0] <= ... <= x[len - 1] (zeros included),
 * and cut = len * (100 - keep_percent) / 200 in integer division, lo = cut, hi = len - cut:
 *     median = x[(len - 1) / 2] (the LOWER median)     low = x[lo]     high = x[hi - 1]     trimmed_sum = x[lo] + ... + x[hi - 1]
 * trimmed_sum / (hi - lo) is the truncated average depth ("TAD80" at keep_percent 80); divided by the genome equivalents of the README's
 * "Normalization" it estimates the gene's copies per genome.  Exact integers, whatever the batches, ranges and launch geometry; a sequence
 * without reads has four zeros.  keep_percent 100 gives trimmed_sum == spanned of mc_coverage_read; low <= median <= high <= max_depth.
 * One selection kernel per call, a workgroup per sequence (csrc/k_depthstats.h): no residue's depth leaves the device - the other route,
 * mc_coverage_depth and a sort on the host, copies all of them.  any != 0 reads the any-depth of mc_set_ties instead (the sequences with
 * candidates are walked).  Arrays of mc_abundance_count() values; any of the four may be NULL.  The state is only read: ranges may follow.
 * Refused, with a message naming the value: keep_percent outside 1 .. 100; coverage off; any != 0 while ties are off; a range in flight. */
int mc_depth_stats(mc_handle *h, int32_t keep_percent, int any, int64_t *median /* [nseq] */, int64_t *trimmed_sum /* [nseq] */, int64_t *low /* [nseq] */,
                   int64_t *high /* [nseq] */);
/* Milliseconds the selection kernels of mc_depth_stats took since the last reset (HIP events) - the device cost of the depth columns beside the
 * README's "Normalization" numerators. */
float mc_depth_stats_ms(const mc_handle *h);

#ifdef __cplusplus
}
#endif
#endif
