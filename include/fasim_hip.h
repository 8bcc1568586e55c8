/* include/fasim_hip.h -- C-ABI of libfasim_hip.so: the MI355X (gfx950) drop-in for the striped
 * Smith-Waterman hot path of Fasim-LongTarget.
 *
 * The reference has no plugin registry; its native boundary for this path is the extern "C" block of
 * ssw.h (ssw.h:19-197) plus, one level up, calc_score_once() (stats.h:879) and fastSIM() (fastsim.h:158)
 * called from LongTarget() (Fasim-LongTarget.cpp:379-598).  Each entry point below names what it replaces.
 * Plain pointers and sizes only; all pointers are HOST pointers unless the name says `_dev`.
 * Every function returns 0 on success or a negative FASIM_E_* code; fasim_last_error() gives the text.
 * There is NO CPU fallback behind this ABI: without a usable HIP device fasim_engine_create() fails.
 */
#ifndef FASIM_HIP_H
#define FASIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASIM_OK            0
#define FASIM_E_NODEVICE   -1   /* no HIP device / HIP runtime error at init                      */
#define FASIM_E_ARG        -2   /* bad argument (null, empty query, letters outside ACGTUN, ...)   */
#define FASIM_E_HIP        -3   /* HIP runtime error (message has the hipError string)             */
#define FASIM_E_OVERFLOW   -4   /* a score left the 16-bit range the path computes in              */
#define FASIM_E_UNSUPPORTED -5  /* input hits behaviour the reference leaves undefined (see DESIGN) */
#define FASIM_E_NOMEM      -6

/* Longest query of the fastSIM entry points.  The reference has no length check; its stage-1 pass (calc_score_once,
 * stats.h:879-956) runs the 16-bit kernel whenever the 8-bit score reaches 255, in the fixed workspace of init_work
 * (stats.h:397): 3 * 16 * (MAXTST + MAXLIB + 32) = 553 536 bytes, of which a 16-bit pass uses 3 * ceil(m / 8) vectors of
 * 16 bytes.  That holds m <= 92 256; above it the reference overruns its heap and its output is undefined, so longer
 * queries get FASIM_E_UNSUPPORTED before any GPU work.  (-F, classic SIM, keeps its own limit of 65 534 nt.) */
#define FASIM_MAX_QUERY 92256

typedef struct fasim_engine fasim_engine;

/* Defaults of initEnv() (Fasim-LongTarget.cpp:284-303); field meaning = struct para (fastsim.h:22-45). */
typedef struct fasim_params {
	int32_t rule;            /* -r   0 = all rules                         */
	int32_t cutLength;       /* -c   5000                                  */
	int32_t strand;          /* -t   0 both, 1 parallel only, -1 anti only */
	int32_t overlapLength;   /* -o   100                                   */
	int32_t ntMin;           /* -ni  20                                    */
	int32_t ntMax;           /* -na  100000                                */
	float   scoreMin;        /*      0                                     */
	float   minIdentity;     /* -i   60   (parsed with atoi by the CLI)    */
	float   minStability;    /* -S   1    (parsed with atoi by the CLI)    */
	int32_t penaltyT;        /* -pt  -1000                                 */
	int32_t penaltyC;        /* -pc  0                                     */
	int32_t cDistance;       /* -ds  15                                    */
	int32_t cLength;         /* -lg  50                                    */
	int32_t classicSim;      /* -F   0; 1 = classic SIM instead of fastSIM (doFastSim = false, Fasim-LongTarget.cpp:360-362) */
} fasim_params;

void fasim_params_default(fasim_params* p);

/* ---- engine ---------------------------------------------------------------------------------- */
/* Process-wide side effects of the first fasim_engine_create() (each can be switched off by its environment variable):
 *   GPU_MAX_HW_QUEUES=8 is exported if unset (the batches in flight need their own hardware queues);
 *   hipSetDeviceFlags(hipDeviceScheduleBlockingSync) for `device`, so that host threads sleep instead of polling in stream
 *     synchronisation (no effect if the host application created the device's context first; FASIM_BLOCKING_SYNC=0);
 *   mallopt(): freed host blocks of up to 32 MB stay in the heap instead of being unmapped -- unmapping host memory while HIP
 *     queues are live stalls the running kernels (FASIM_MALLOPT=0). */
int  fasim_engine_create(int device, fasim_engine** out);
/* flags = FASIM_CREATE_NO_PROCESS_TUNING: none of the three process-wide settings above is touched (what a host application that
 * only embeds single calls wants; the `ssw.h` symbols create their engine this way).  The worker engines of a scan inherit nothing:
 * they are created by the scan through fasim_engine_create, so a throughput run should create its engine without the flag. */
#define FASIM_CREATE_NO_PROCESS_TUNING 1
int  fasim_engine_create_ex(int device, int32_t flags, fasim_engine** out);
void fasim_engine_destroy(fasim_engine* e);
const char* fasim_last_error(const fasim_engine* e);   /* e may be NULL: last global error */

/* Tuning knobs (optional).  key "workers": batches kept in flight by fasim_scan (default 10, env FASIM_WORKERS);
 * key "seg_batch": segments per batch (default 384; a single-lncRNA scan of >= 128 segments per worker gets batches fitted to the
 * record instead, at most 512 segments, -F 16 ... 128; env FASIM_SEG_BATCH); value <= 0 restores the default.
 * key "taper": percent of the segments scanned in half-size batches at the end (default: 25 for a single-lncRNA scan whose batches are fitted to the record, else 0);
 * key "heavy_gate": k_scan / k_align_fwd launches in flight at once (default 4, env FASIM_HEAVY_GATE; 0 = no gate);
 * -1 restores the default of the last two.
 * key "host_threads": host threads for the host side of the batches, all workers of this engine together (default 3/8 of the
 * cores, at most 96, env FASIM_HOST_THREADS); several engines in one process should share the cores.
 * key "hazard_chunks" (1) / "hazard_snapshots" (0) / "hazard_chunk_cols" (200) / "hazard_hot_weight" (2): the stripe-faithful
 * re-run of the units the reference's signed lazy-F exit can touch: in parallel column chunks from checkpoints (0: one
 * sequential run per unit), checkpoint pass continued from pipeline snapshots of the main scan (0: from column 0; the snapshots
 * cost 64 KB of HBM writes per unit), cost target of a chunk in columns, price of a column whose maximum is >= 144
 * (env FASIM_HAZARD_CHUNKS, FASIM_HAZARD_SNAP).
 * key "striped_window" (0): 1 runs every stripe-faithful (k_striped) launch on its HBM-window variant, which otherwise serves only
 * the queries whose stripes do not fit the LDS (env FASIM_STRIPED_WINDOW; for tests: results do not depend on it).
 * key "site_short" (1): fasim_scan_oligos_aligned finds the end and start cell of every hit with k_site_ends_short, one problem per
 * lane over a window of the unit (csrc/site_short.hip); 0 = with k_site_ends, one workgroup per problem over the unit's prefix (env
 * FASIM_SITE_SHORT; results do not depend on it).  key "site_chunk" (0): problems per chunk of the hits phase of
 * fasim_scan_records_sites_aligned and fasim_scan_oligos_aligned where it is lower than the phase's own limit (4 096, oligos 262 144;
 * value <= 0 restores those; results do not depend on it).
 * key "numa_affinity" (1): for the duration of a scan the calling thread and the threads the scan starts are pinned to the CPUs of
 * the GPU's NUMA node (/sys/bus/pci/devices/<bus id>/local_cpulist); the caller's affinity is restored afterwards; no effect on a
 * single-node machine.
 * key "band" (1): the banded forward pass of stage 3 (csrc/band.hip); 0 = every window try runs over the whole query (env FASIM_BAND).
 * key "q2_past_cut" (0): 0 = k_scan stops tracking the taints of the reference's signed lazy-F exit (Q2) in a unit 128 pipeline
 * steps after a block of 64 steps whose maximum is >= 251 and clean: such a value proves the unit's overflow cut, and no taint behind
 * the cut is ever read (csrc/scan.hip); 1 = it tracks to the end of every unit, as before the option existed;
 * -1 restores the default (env FASIM_Q2_PAST_CUT).  Results, hazard units and every counter do not depend on it: only bit 0 of
 * k_scan's column maxima behind the cut does (tests/test_gpu_q2_past_cut.py).
 * key "finish_skip" (1): 1 = the finish of fasim_scan and its kin (k_finish_rev / k_finish_trace, csrc/align.hip) leaves an alignment
 * without its CIGAR when its record is certain to fail the stability filter (csrc/doomed.h, DESIGN.md section 2: a TT pair on the
 * display strand inside the alignment's span under penaltyT < 0, minStability > 0), counted in stats.finish_skipped; 0 = k_finish_lds
 * traces every alignment, as before the option existed; 2 = every alignment is traced and the rule is checked against the full
 * conversion, misses counted in stats.finish_skip_violations; -1 restores the default (env FASIM_FINISH_SKIP).  The records do not
 * depend on it (tests/test_gpu_finish_skip.py).  fasim_align_batch* return CIGARs and never skip.
 * key "sim_lds" (-1): which storage variant of k_sim_resweep the -F rounds launch.  -1 = by the units in flight (the LDS variant
 * once at most 256 are left over all workers); 0 = always the variant that keeps the lines' states in L2; 1 = always the LDS variant
 * (the kernel still takes the L2 variant when the states of a unit exceed 150 KB).  No environment variable (for tests).
 * Results do not depend on any of them. */
int fasim_set_option(fasim_engine* e, const char* key, int32_t value);

/* Replaces ssw_init()/init_destroy() (ssw.h:78,83) and init_work() (stats.h:386): the lncRNA is
 * encoded once and stays resident on the device (the reference rebuilds its profile on every call). */
int fasim_set_query(fasim_engine* e, const char* rna, int32_t len);

/* ---- single-problem drop-ins of the native kernels (each launches the HIP path) --------------- */
/* calc_score_once() (stats.h:879-956): exact max local score of the query vs `target`.            */
int fasim_calc_score_once(fasim_engine* e, const char* target, int32_t n, int32_t* score);
/* ssw_pre_align() (ssw.h:128, sswNew.cpp:1309) behind Aligner::preAlign's base translation
 * (ssw_cpp.cpp:394-415): out_cols[n] = per-column maxima incl. the reference's Q1/Q2/Q3 behaviour. */
int fasim_ssw_pre_align(fasim_engine* e, const char* target, int32_t n, int32_t* out_cols);
/* column maxima of the reference's 16-bit kernels (sw_sse2_word, sswNew.cpp:893-1069; same DP as the unreachable
 * sw_sse2_word_once, :698): 8 stripes, no overflow rule, no signed-compare quirk.  Used by the ssw.h shim
 * (include/ssw.h) for the sub-optimal score of alignments whose score overflows 8 bits.                */
int fasim_ssw_colmax_word(fasim_engine* e, const char* target, int32_t n, int32_t* out_cols);
/* peak picking of Aligner::preAlign (ssw_cpp.cpp:427-572) on a column-max array (host logic).     */
int fasim_pick_candidates(const int32_t* cols, int32_t n, int32_t threshold,
                          int32_t* out_score, int32_t* out_pos, int32_t cap, int32_t* count);
/* Self-check of the host record path (pure host code, no device): `n` random alignments (random CIGARs over a random segment
 * and lncRNA, every rule encoding) through the numbers-only conversion the scan uses and through the reference-shaped
 * string conversion, then both record types through the dedup (sort / unique with the reference's comparators, which are
 * not strict weak orderings: the order must match exactly).  *mismatches = number of differences (0 expected).          */
int fasim_selfcheck_records(uint64_t seed, int32_t n, int32_t* mismatches);
/* v_pk_maximum3_f16 as the f16 DP kernels use it (option dp_f16), on the engine's device: for n packed f16 pairs
 * out3[i] = maximum3(a[i], b[i], c[i]) and out0[i] = maximum3(a[i], b[i], +0) (the inline constant).  For tests: on
 * integer-valued operands both must be the integer maximum, bit for bit.                                             */
int fasim_maximum3_f16(fasim_engine* e, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out3, uint32_t* out0, int64_t n);
/* ssw_align() (ssw.h:118, sswNew.cpp:1446) behind Aligner::Align (ssw_cpp.cpp:599-643).           */
typedef struct fasim_alignment {
	int32_t sw_score, ref_begin, ref_end, query_begin, query_end;
	int32_t cigar_len;                 /* number of BAM-encoded ops in cigar[]; -1 (with sw_score 0): the
	                                      reference's ssw_align returns NULL here (banded_sw finds no path,
	                                      sswNew.cpp:1535-1538), which its callers treat as score 0      */
	uint32_t cigar[256];               /* (len<<4)|op, op 0=M 1=I 2=D (ssw.h:174)                   */
} fasim_alignment;
int fasim_ssw_align(fasim_engine* e, const char* window, int32_t n, fasim_alignment* out);
/* batched forms (the shapes the engine uses internally): nprob problems, targets concatenated      */
int fasim_pre_align_batch(fasim_engine* e, const char* targets, const int64_t* offsets, const int32_t* lens,
                          int32_t nprob, int32_t* out_cols /* concatenated like targets */, int32_t* out_stage1);
int fasim_align_batch(fasim_engine* e, const char* windows, const int64_t* offsets, const int32_t* lens,
                      int32_t nprob, fasim_alignment* out);
/* The same call; path[i] (path may be NULL) tells which part of the engine produced alignment i:
 *   0 nothing aligned (forward score 0);
 *   1 k_finish_lds<64, 2048> (16 KB of LDS), 2 k_finish_lds<256, 16384> (64 KB of LDS),
 *   3 k_finish with 16 KB of global scratch, 4 k_finish with 1 MB of global scratch;
 *   5 the stripe-faithful replay (also every window when the query or a window does not fit the systolic kernels).  */
int fasim_align_batch_ex(fasim_engine* e, const char* windows, const int64_t* offsets, const int32_t* lens,
                         int32_t nprob, fasim_alignment* out, int32_t* path /* [nprob], may be NULL */);
/* transferString()/reverseSeq()/complement() (rules.h:59-318) for encoding enc in [0,48), canonical
 * execution order of LongTarget(): target[n] and src[n] (src is NUL-padded if letters were dropped). */
int fasim_encode_unit(const char* seg, int32_t n, int32_t enc, char* target, char* src);

/* ---- row f3: the -F path, classic SIM (sim.h:410-1143) ------------------------------------------- */
/* The forward sweep of SIM() (sim.h:506-571) on the GPU: local alignment scores with start points over the whole
 * (query x target) matrix, every cell above `min_score` fed to the K = 50 node list in row-major order (addnode,
 * sim.h:99-148).  Returns the node list the sweep leaves, in list order: what the reference holds when its traceback
 * loop starts (sim.h:572).  Scores are the reference's x10 values; min_score is compared unscaled, as the reference
 * does (sim.h:567).  fasim_scan with params.classicSim = 1 runs the whole -F path: this sweep on the GPU, then K rounds in
 * lock step over the units of a batch -- best node, linear-space traceback and triplex record on host threads
 * (csrc/host_sim.cpp), the backward / growing / forward re-sweeps of the influenced rectangles (sim.h:884-1141) on the GPU
 * (k_sim_resweep, csrc/sim.hip).
 * Query and targets: ACGT (other letters score as mismatches; the reference reads an uninitialised table there), at most
 * 65534 long (16-bit start fields in the 64-bit DP keys; a re-sweep starts lines at row M + 1 / column N + 1). */
typedef struct fasim_sim_node { int64_t score, stari, starj, endi, endj, top, bot, left, right; } fasim_sim_node;
#define FASIM_SIM_K 50
typedef struct fasim_result fasim_result;      /* defined below */
/* Host half of the -F path for ONE unit (pure host code, no device): everything SIM() does after its first sweep
 * (sim.h:572-1141) for segment `seg` under encoding `enc`, starting from the node list of the forward sweep.  The records
 * are the unit's triplexes as SIM() appends them (before LongTarget()'s tail filter). */
int fasim_sim_finish_unit(const char* rna, int32_t m, const char* seg, int32_t n, int32_t enc, int64_t dna_start, int64_t min_score,
                          const fasim_params* p, const fasim_sim_node* nodes, int32_t nnodes, fasim_result** out);
int fasim_sim_forward_batch(fasim_engine* e, const char* targets, const int64_t* offsets, const int32_t* lens, int32_t nprob,
                            const int64_t* min_scores, fasim_sim_node* nodes /* [nprob][FASIM_SIM_K] */, int32_t* counts /* [nprob] */);

/* ---- the batched body of LongTarget() (Fasim-LongTarget.cpp:379-598) -------------------------- */
/* One record per triplex that survives fastSIM()'s own filter and LongTarget()'s tail filter, in the
 * reference's order (segment, encoding, fastSIM rank).  Strings live in `pool` (NUL-terminated).   */
typedef struct fasim_triplex {
	int32_t stari, endi, starj, endj, strand, reverse, rule, nt;
	float   score, identity, tri_score;
	int32_t seg, enc;                   /* provenance: segment index, encoding index                 */
	int32_t genome_shift;               /* added to start_genome for THIS record's genome coordinates; 0 from
	                                       fasim_scan.  Only the B1-compatible reader (--accumulate-records) sets it:
	                                       the reference patches each FASTA record's triplexes with that record's
	                                       own start (Fasim-LongTarget.cpp:141-149)                         */
	int64_t tfo_off, tts_off;           /* offsets of stri_align / strj_align in pool                */
} fasim_triplex;

#define FASIM_KERNEL_FAMILIES 10
typedef struct fasim_scan_stats {
	int64_t segments, segments_skipped, units;
	int64_t candidates, align_calls;
	int64_t align_word_reruns;          /* window alignments repeated with the 16-bit pass (8-bit maximum >= 251) */
	int64_t stage2_overflow_units, stage1_word_reruns;
	int64_t logical_cells;              /* m * sum(len(segment)) * n_enc                  */
	double  t_total_s, t_stage1_s, t_stage2_s, t_stage3_s, t_host_s;   /* host wall clock per phase       */
	/* HIP-event time of the kernels, summed over launches (each on the stream it was launched on; with several
	 * batches in flight the durations include sharing the GPU).  index: 0 k_scan (fused stage 1+2), 1 k_striped
	 * stage-1/2 (hazard re-runs, long queries), 2 k_align_fwd, 3 k_finish_lds, 4 encode/hits/post/stream,
	 * 5 k_striped stage 3 (exact replays, exact reverse passes), 6 k_finish (global scratch) + k_banded, 7 k_sim_forward (-F) */
	double  kernel_ms[FASIM_KERNEL_FAMILIES];      /* ... 8 k_align_band (banded stage-3 forward), 9 k_band_select */
	int64_t kernel_launches[FASIM_KERNEL_FAMILIES];
	int64_t cells_stage1, cells_stage2, cells_stage3;   /* DP cells actually executed (stage 3: fwd + rev)   */
	int64_t hazard_units;               /* units re-run by the stripe-faithful kernel (possible Q2)  */
	int64_t rev_exact;                  /* window tries whose reverse pass ran on the stripe-faithful kernel */
	int64_t exact_replays;              /* candidates replayed try by try on the stripe-faithful kernels */
	int64_t tries_skipped;              /* window tries of the reference whose result cannot matter and that were not run */
	int64_t band_tries;                 /* forward passes run on a row band (k_align_band), second attempts included */
	int64_t band_proven;                /* window tries whose band result was proven to be the full-height result */
	int64_t band_cells;                 /* DP cells executed by k_align_band (part of cells_stage3) */
	int64_t rev_bound_passes;           /* window tries that took the full-height reverse pass (bounds for the band passes) */
	int64_t striped_window_probs;       /* problems run on the HBM-window variant of k_striped (query stripes too long for the LDS) */
	double  striped_window_ms;          /* HIP-event time of those launches (also counted in kernel_ms[1] / kernel_ms[5]) */
	int64_t dp_f16_reruns;              /* units whose scores left the exact range of the f16 k_scan (>= 1 024) and that the integer k_scan ran again */
	/* alignments of the scan's finish (run_finish) by the storage tier that answered them: k_finish_lds with 16 KB and with
	 * 64 KB of LDS, k_finish with 16 KB and with 1 MB of global scratch per alignment */
	int64_t finish_lds16, finish_lds64, finish_glob16k, finish_glob1m;
	/* -F: launches of k_sim_resweep by storage variant (lines' states in LDS / in L2); unit-launches that came back suspended (budget
	 * or time slice spent before the re-sweep ended); suspended units that were resumed by the other variant than the one that
	 * suspended them */
	int64_t sim_resweep_lds, sim_resweep_l2, sim_suspended, sim_handover;
	/* option finish_skip: alignments of the scan's finish left without a CIGAR because the stability filter is certain to drop
	 * their record (mode 2: that would have been left); mode 2 only: those for which the full conversion did not confirm it */
	int64_t finish_skipped, finish_skip_violations;
} fasim_scan_stats;

struct fasim_result {
	fasim_triplex* recs; int64_t count;
	char* pool; int64_t pool_len;
	fasim_scan_stats stats;
};

/* Scans segments [seg_first, seg_first+seg_count) of `dna` (whole sequence of ONE FASTA record, host
 * memory, upper-case ACGTN).  Coordinates in the records are relative to the whole `dna` exactly as in
 * the reference.  seg_count < 0 = all remaining.  Used unsharded (1 GPU) or per rank (multi-GPU).   */
int fasim_scan(fasim_engine* e, const char* dna, int64_t dna_len, int64_t seg_first, int64_t seg_count,
               const fasim_params* p, fasim_result** out);
/* Multi-lncRNA batch (BASELINE config 4: many lncRNAs x one genome).  The reference holds ONE RNA per run
 * (readRna(), Fasim-LongTarget.cpp:174-200) and is started once per lncRNA; here the DNA record stays resident
 * and every (lncRNA, batch of segments) pair is one work item of the same queue, so consecutive lncRNAs overlap
 * instead of paying a ramp-up and a drain each.  out[q] receives the records of rnas[q] exactly as fasim_scan
 * would return them for that query alone (free each with fasim_result_free).  dna == NULL scans the resident
 * record (fasim_load_dna).  Afterwards the engine's current query is rnas[nq-1].  Per-result stats.t_total_s is
 * the wall clock from the start of that query's first batch to the end of its last one (neighbours overlap). */
int fasim_scan_queries(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                       const char* dna, int64_t dna_len, int64_t seg_first, int64_t seg_count,
                       const fasim_params* p, fasim_result** out /* [nq] */);
/* Record sets (ChIP / ChIRP peaks, promoter windows, enhancers): many short DNA records scanned in shared batches.
 * Record r is dna[rec_off[r] .. rec_off[r] + rec_len[r]) in host memory; dna == NULL: the offsets refer to the resident buffer
 * of fasim_load_dna.  nq == 0: the engine's current query (as fasim_scan); nq > 0: as fasim_scan_queries.
 * Each record is cut into segments exactly as fasim_scan cuts that record alone (fasim_segment_count(rec_len[r])); the
 * segments are then numbered globally, record after record, and [seg_first, seg_first + seg_count) picks a contiguous range of
 * that list (seg_count < 0: to the end), so a record set is sharded like one record.  A batch may cross records.
 * out[q * nrec + r] is, byte for byte, what fasim_scan with query q returns for record r alone, restricted to the selected
 * segments of that record: the same triplex records in the same order, `seg` = segment index within the record,
 * genome_shift 0, the same pool bytes.  A record with no selected segment gets an empty result.
 * Per-record stats: segments, segments_skipped, units, candidates, align_calls, logical_cells and cells_stage2 equal the
 * single-record scan's (all counted per unit or per candidate); every other field is zero.  totals[q] (may be NULL) holds the
 * sums of all fields over the call and the query's wall clock in t_total_s.
 * Refused with FASIM_E_ARG before any GPU work, the record index in fasim_last_error: nrec < 1; a negative offset; a record
 * outside the resident buffer (a host buffer has no length here: the caller guarantees that `dna` holds every record); a
 * record of length 0 (fasim_scan refuses it too); a record longer than 2^31 - 1 nt.  A query above FASIM_MAX_QUERY gets
 * FASIM_E_UNSUPPORTED, and classicSim (-F) keeps its own limits.  The engine stays usable after a refusal.  The whole set
 * may be longer than 2^31 nt; only one record is limited.  Free every result with fasim_result_free.
 * The slices need not lie back to back: records may overlap, nest, repeat and come in any order, in a host buffer and in the
 * resident buffer alike (BED intervals of one chromosome, Engine.scan_regions); each is still scanned as that slice alone. */
int fasim_scan_records(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                       const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                       int64_t seg_first, int64_t seg_count, const fasim_params* p,
                       fasim_result** out /* [nq * nrec] (nq == 0: [nrec]), query-major */,
                       fasim_scan_stats* totals /* [nq] (nq == 0: [1]), may be NULL */);
/* ---- per-base triplex potential tracks (csrc/track.hip) ------------------------------------------------ */
/* What the scan computes for every base and the candidate threshold (80 % of the unit's stage-1 maximum) hides: per strand class
 * and record bin the best local alignment score of the lncRNA that ends in the bin.  Class = the Strand column of -TFOsorted.
 * v[c][b] = maximum over the units (segment x encoding) of class c and over the record positions x in [b * bin, (b + 1) * bin) of
 * the unit's column maximum at x: textbook Gotoh local alignment with the stage-2 scoring (+5 / -4, N = mismatch, gap 16 + 4 per
 * further residue, the reference's zero-score pad rows), WITHOUT the reference's 8-bit overflow cut (Q1) and lazy-F deviation (Q2);
 * 0 where no unit covers x (segments skipped as one repeated letter, disabled classes, segments outside the selected range).
 * Scores saturate at 16 383: a unit that reaches it reports 16 383 there and lower bounds after it (saturated_units counts them). */
#define FASIM_TRACK_CLASSES 4      /* 0 ParaPlus 1 ParaMinus 2 AntiMinus 3 AntiPlus */
typedef struct fasim_track {
	int64_t nbins; int32_t bin;                 /* nbins = ceil(dna_len / bin)            */
	uint16_t* v[FASIM_TRACK_CLASSES];            /* nbins values each                      */
	int64_t units, saturated_units;
} fasim_track;
/* Shape of fasim_scan_queries (nq == 0: the engine's current query; dna == NULL: the resident record).
 * out_results == NULL: track only, stage 3 is not run.  Otherwise out_results[q] is byte for byte what
 * fasim_scan_queries returns.  out_tracks[q]: free with fasim_track_free.
 * With a segment range only the selected segments contribute and the arrays still span the whole record, so the tracks of shards
 * are merged by fasim_track_merge.  The values come from the systolic scan kernel only.  Refused before any GPU work, the engine
 * stays usable: bin < 1 or out_tracks == NULL (FASIM_E_ARG); a query shorter than 113 nt, an engine created under FASIM_SCAN_V1=1,
 * classicSim = 1 (FASIM_E_UNSUPPORTED, the reason in fasim_last_error). */
int  fasim_scan_track(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                      const char* dna, int64_t dna_len, int64_t seg_first, int64_t seg_count, const fasim_params* p,
                      int32_t bin, fasim_result** out_results, fasim_track** out_tracks);
/* Element-wise maximum of `nparts` tracks of one record (shards, devices); units and saturated_units are summed.  Parts whose bin
 * or nbins differ are refused (FASIM_E_ARG).  Free the result with fasim_track_free. */
int  fasim_track_merge(const fasim_track* const* parts, int32_t nparts, fasim_track** out);
/* bedGraph text: four `track type=bedGraph name='<rna> potential (<class>)'` blocks in class order, 0-based half-open genome
 * coordinates (start_genome as in fasim_tfoclass: the 1-based genome position of the record's first base), one line
 * `<chr>\t<start>\t<end>\t<value>` per run of equal neighbouring bins, the last bin clipped to dna_len, bins below min_value
 * (>= 1, so zeros never appear) left out.  dna_len must be the record length the track was made for.  Free with fasim_free. */
int  fasim_track_bedgraph(const fasim_track* t, const char* chr, int64_t start_genome, int64_t dna_len,
                          const char* rna_name, int32_t min_value, char** text, int64_t* text_len);
void fasim_track_free(fasim_track* t);
/* ---- record sets and BED intervals screened by potential ------------------------------------------------ */
/* Peak of one (record, class): value = the maximum of the record's per-base potential P[c][x] (the bin = 1 track of the record
 * scanned alone), pos = the smallest record position x (0-based) that attains it, enc = the smallest enabled encoding index of the
 * class for which a unit covering pos attains it at pos.  value == 0: pos = enc = -1.  A function of the record and the parameters
 * only (not of batches, workers, shards, devices or dp_f16, nor of whether tracks or stage 3 were asked for). */
typedef struct fasim_peak { int32_t value, enc; int64_t pos; } fasim_peak;
/* fasim_scan_records with the potential of every record: arguments, record cutting, global segment numbering and the refusals of
 * fasim_scan_records, plus those of fasim_scan_track (a query under 113 nt, FASIM_SCAN_V1=1, classicSim: FASIM_E_UNSUPPORTED).
 * Indexing is [q * nrec + r] (peaks: [(q * nrec + r) * 4 + c]; nq == 0: the engine's query, q = 0).
 * bin == 0: peaks only (out_tracks must be NULL, out_peaks must not): the kernel writes no track slices and only the slices'
 * peaks come back.  bin >= 1: out_tracks[q * nrec + r] is one fasim_track spanning record r, exactly what fasim_scan_track gives
 * for that record alone restricted to the selected segments (free each with fasim_track_free); out_peaks may be NULL.  bin < 0:
 * FASIM_E_ARG.  out_results == NULL: no stage 3 (the work ends after the scan kernel and k_track); otherwise out_results and
 * totals are byte for byte those of fasim_scan_records.  With a segment range only the selected segments contribute: merge the
 * shards with fasim_track_merge / fasim_peaks_merge.  Every refusal happens before any GPU work and leaves the engine usable. */
int fasim_scan_records_track(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                             const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                             int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t bin,
                             fasim_result** out_results /* [nq * nrec] or NULL */, fasim_track** out_tracks /* [nq * nrec] or NULL */,
                             fasim_peak* out_peaks /* [nq * nrec * 4] or NULL */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* Entry-wise merge of `nparts` arrays of n peaks each (shards, devices): the larger value wins, then the lower pos, then the lower
 * enc.  (0, -1, -1) entries therefore lose against every peak of value >= 1. */
int fasim_peaks_merge(const fasim_peak* const* parts, int32_t nparts, int64_t n, fasim_peak* out);
/* ---- per-base profile of the lncRNA (csrc/rowfold.hip) ---------------------------------------------------- */
/* The other projection of the scan's matrices: for every base of the lncRNA and strand class the best local alignment score that
 * ends ON THAT BASE, anywhere in the records -- which stretch of the lncRNA is the triplex-forming domain.  v[c][i] = maximum over
 * the selected units of class c and over their real columns of H[i][j] of section 11 (the textbook values of the potential
 * tracks: no 80 % threshold, no Q1, no Q2); 0 where no unit contributes.  The query is never reversed: row i is base i for every
 * encoding.  Saturation at 16 383 as for the tracks.  max_i v[c][i] equals the maximum of the class's potential track. */
typedef struct fasim_tfo_profile {
	int32_t m;                                   /* bases of the lncRNA                    */
	uint16_t* v[FASIM_TRACK_CLASSES];            /* m values each                          */
	int64_t units, saturated_units;
} fasim_tfo_profile;
/* fasim_scan_records with the profile: arguments, record cutting, global segment numbering and the refusals of fasim_scan_records,
 * plus those of fasim_scan_track (a query under 113 nt, FASIM_SCAN_V1=1, classicSim: FASIM_E_UNSUPPORTED), all before any GPU work;
 * the engine stays usable.  per_record == 0: out_profiles[q] is one profile per query over the whole record set; otherwise
 * out_profiles[q * nrec + r] is the profile of record r, exactly what that record scanned alone gives.  out_results == NULL: no
 * stage 3 (the work ends after the scan kernel and k_rowfold); otherwise out_results and totals are byte for byte those of
 * fasim_scan_records.  With a segment range only the selected segments contribute: merge the shards with
 * fasim_tfo_profile_merge.  The result depends on the records and the parameters only (not on batches, workers, shards, devices or
 * dp_f16, nor on whether stage 3 ran).  Free each profile with fasim_tfo_profile_free. */
int  fasim_scan_tfo_profile(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                            const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                            int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t per_record,
                            fasim_result** out_results /* [nq * nrec] or NULL: no stage 3 */,
                            fasim_tfo_profile** out_profiles /* [nq] or, per_record, [nq * nrec] */,
                            fasim_scan_stats* totals /* [nq], may be NULL */);
/* Element-wise maximum of `nparts` profiles of one lncRNA (shards, devices); units and saturated_units are summed.  Parts whose m
 * differ, and an empty list, are refused (FASIM_E_ARG).  Free the result with fasim_tfo_profile_free. */
int  fasim_tfo_profile_merge(const fasim_tfo_profile* const* parts, int32_t nparts, fasim_tfo_profile** out);
/* The table `fasim --tfo-profile` writes: the header line `pos base ParaPlus ParaMinus AntiMinus AntiPlus`, then one line per base
 * of `rna` (t->m letters, written as given), all tab-separated, pos 1-based.  rna_name may be NULL.  Free with fasim_free. */
int  fasim_tfo_profile_tsv(const fasim_tfo_profile* t, const char* rna, const char* rna_name, char** text, int64_t* text_len);
void fasim_tfo_profile_free(fasim_tfo_profile* t);
/* ---- sites above a fixed potential (csrc/sites.hip) -------------------------------------------------------- */
/* Where in the record the potential reaches min_value.  P[c][x] is the bin = 1 track of section 11 of the record scanned alone.  A raw
 * run of class c is a maximal range [a, b) of positions with P[c][x] >= min_value; a SITE is the union of a maximal chain of raw runs
 * of one class in which every run starts at most max_gap positions after the end of the one before it.  start / end are 0-based
 * half-open record positions, value the maximum of P[cls] over [start, end), pos the smallest position that attains it and enc the
 * peak rule of section 12: the smallest enabled encoding of the class one of whose units covering pos attains value there.  The
 * sites of a record are ordered by (start, cls).  Unlike the candidate threshold of -TFOsorted (80 % of the unit's own maximum),
 * min_value is absolute: a site does not depend on what else lies in its segment.  A record and class have no site iff their peak
 * (fasim_scan_records_track, bin 0) is below min_value; otherwise the site of the largest value, first on ties, carries the peak's
 * (value, pos, enc). */
typedef struct fasim_site  { int64_t start, end, pos; int32_t value, enc, cls, reserved; } fasim_site;
typedef struct fasim_sites {
	int64_t n; fasim_site* s;                    /* n sites, ordered by (start, cls)                                        */
	int64_t units, saturated_units;              /* as fasim_track                                                          */
	int64_t raw_runs;                            /* runs the kernel left for this record (cut at slice and segment edges)   */
	int32_t min_value, max_gap;
} fasim_sites;
/* fasim_scan_records with the sites: arguments, record cutting, global segment numbering and the refusals of
 * fasim_scan_records_track (one record is the nrec = 1 case, dna == NULL the resident buffer; with dna == NULL and nrec == 1,
 * rec_off == NULL and rec_len == NULL stand for the whole resident buffer as one record).  In addition min_value < 1,
 * min_value > 16383, max_gap < 0 or out_sites == NULL give FASIM_E_ARG; a query under 113 nt, FASIM_SCAN_V1=1 or classicSim give
 * FASIM_E_UNSUPPORTED.  Every refusal happens before any GPU work and leaves the engine usable, as does FASIM_E_NOMEM when the run
 * buffers cannot be allocated.  out_results == NULL: no stage 3 (the work ends after the scan kernel and k_sites); otherwise
 * out_results and totals are byte for byte those of fasim_scan_records.  out_sites[q * nrec + r] depends on the record, the query,
 * the parameters, min_value and max_gap only (not on batches, workers, shards, devices, dp_f16, resident or streamed DNA, nor on
 * whether stage 3 ran).  With a segment range only the selected segments contribute: merge the shards of a record with
 * fasim_sites_merge.  Free each with fasim_sites_free. */
int  fasim_scan_records_sites(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                              const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                              int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t min_value, int32_t max_gap,
                              fasim_result** out_results /* [nq * nrec] or NULL: no stage 3 */,
                              fasim_sites** out_sites /* [nq * nrec] */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* Shards of ONE record: the union of the parts' intervals per class, joined by max_gap again -- the list of the unsharded call.
 * Where intervals unite the larger value wins, then the smaller pos, then the smaller enc; units, saturated_units and raw_runs are
 * summed.  Parts whose min_value or max_gap differ, and an empty list, are refused (FASIM_E_ARG). */
int  fasim_sites_merge(const fasim_sites* const* parts, int32_t nparts, fasim_sites** out);
/* BED text of a site list.  header != 0: first the line `# fasim sites lncRNA=<rna_name> min_value=<V> max_gap=<G>`.  Then one
 * tab-separated line per site: chrom, start, end, class name, value, strand (+ for ParaPlus / AntiPlus, - for ParaMinus /
 * AntiMinus), peak, rule (the Rule column of -TFOsorted for enc), and record_name as a ninth column where it is not NULL.
 * start, end and peak are 0-based half-open genome coordinates, start_genome - 1 + x, start_genome as in fasim_tfoclass.  Free the
 * text with fasim_free. */
int  fasim_sites_bed(const fasim_sites* t, const char* chr, int64_t start_genome, const char* rna_name,
                     const char* record_name /* NULL: 8 columns */, int32_t header, char** text, int64_t* text_len);
void fasim_sites_free(fasim_sites* t);
/* ---- every site with its hit (csrc/site_align.hip) ---------------------------------------------------------- */
/* The HIT of a site is the textbook local alignment behind its peak: H is the matrix of section 11 (plain Gotoh, +5 / -4, every
 * non-ACGT letter -4, U read as A, gap 16 then 4, floored at 0, no Q1, no Q2).  Unit: the selected segment of the smallest index that
 * covers pos and whose unit under `enc` has column maximum `value` at pos.  End cell (i1, j1): the largest column j1 <= the column
 * of pos at which a real row holds H == value (a pad row only repeats row m - 1 one column later per row), the smallest such row
 * i1.  Start cell (i0, j0): among the alignments that begin with a pair, end with the pair (i1, j1) and score `value`, the largest
 * column j0 and then the largest row i0 -- the alignment that is shortest on the DNA side.  Path: the anchored Gotoh matrices of the
 * rectangle, traced back from (i1, j1) with fixed priorities (in H: diagonal, then E, then F; in a gap state: extend, then open).
 * The alignment then goes through the conversion every record of fasim_scan goes through, with -ni 1 and no -na, and is never
 * filtered: t[k] is the fasim_triplex of site k (score = value; strings in pool), q_begin / q_end / t_begin / t_end the
 * unit-relative cells i0, i1, j0, j1, cigar[cigar_off[k] .. + cigar_len[k]) its CIGAR ((len << 4) | op, 0 = M, 1 = I: a query
 * base against a gap, 2 = D: a target base against a gap; first and last operation M).
 * Limits: a site of value 16 383 (a saturated unit), a site whose unit no longer holds `value` in exact arithmetic (possible only
 * after a saturation), an end cell that no alignment beginning and ending with a pair reaches with `value`, and a hit whose rectangle
 * has more than 8 192 rows or 2^26 cells (4 x 4 096 x 4 096), and every site of a call with cutLength above 6 000, come back with cigar_len = -1, empty strings and whatever cells were
 * found (-1 otherwise), and are counted in `unaligned`. */
typedef struct fasim_site_hits {
	int64_t n; fasim_triplex* t;                 /* n hits: hit k belongs to site k of the same (query, record)            */
	int32_t* q_begin, *q_end, *t_begin, *t_end;  /* i0, i1, j0, j1                                                          */
	int64_t* cigar_off; int32_t* cigar_len; uint32_t* cigar;
	char* pool; int64_t pool_len;
	int64_t unaligned;
} fasim_site_hits;
/* fasim_scan_records_sites and, as a second phase once the sites are final, the hit of every site: the arguments and refusals of
 * fasim_scan_records_sites, plus out_hits == NULL -> FASIM_E_ARG.  out_sites, out_results and totals are byte for byte those of
 * fasim_scan_records_sites.  out_hits[q * nrec + r] depends on the record, the query, the parameters, min_value and max_gap only.
 * FASIM_E_NOMEM leaves the engine usable.  Free each with fasim_site_hits_free. */
int  fasim_scan_records_sites_aligned(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                                      const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                                      int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t min_value, int32_t max_gap,
                                      fasim_result** out_results /* [nq * nrec] or NULL: no stage 3 */,
                                      fasim_sites** out_sites /* [nq * nrec] */, fasim_site_hits** out_hits /* [nq * nrec] */,
                                      fasim_scan_stats* totals /* [nq], may be NULL */);
/* Shards of ONE record: sites[k] / hits[k] are what shard k returned.  *out_sites (may be NULL) receives fasim_sites_merge of the
 * site lists, *out_hits the hits of that merged list: where intervals unite, the part whose site wins (larger value, smaller pos,
 * smaller enc) supplies the hit; on a full tie the hit of the smaller `seg` wins (an unaligned hit loses against an aligned one).
 * Refusals: those of fasim_sites_merge, and a part whose hits->n differs from its sites->n (FASIM_E_ARG). */
int  fasim_site_hits_merge(const fasim_sites* const* sites, const fasim_site_hits* const* hits, int32_t nparts,
                           fasim_sites** out_sites, fasim_site_hits** out_hits);
/* The table `fasim --sites V --sites-align` writes.  header != 0: first `# fasim site hits lncRNA=<rna_name> min_value=<V>
 * max_gap=<G>` and the line of column names.  Then one tab-separated line per site, in the order of the site list: chrom
 * tts_start tts_end class value strand rule tfo_start tfo_end nt identity stability cigar TFO TTS, and record_name as a last
 * column where it is not NULL.  tts_start / tts_end: 0-based half-open genome coordinates of the DNA bases of the hit
 * (start_genome as in fasim_sites_bed); tfo_start / tfo_end: 1-based inclusive lncRNA positions; identity and stability printed as
 * -TFOsorted prints them.  An unaligned hit has NA from rule on (tts_start / tts_end: the site's range).  Free with fasim_free. */
int  fasim_site_hits_tsv(const fasim_sites* s, const fasim_site_hits* h, const char* chr, int64_t start_genome, const char* rna_name,
                         const char* record_name /* NULL: 15 columns */, int32_t header, char** text, int64_t* text_len);
void fasim_site_hits_free(fasim_site_hits* h);
/* ---- panels of short oligos (csrc/scan_short.hip) ----------------------------------------------------------- */
/* Sites and potential tracks of a panel of nq triplex-forming oligos of 1 .. FASIM_MAX_OLIGO nt against one record set.  The
 * potential of an oligo is that of section 11 with the oligo in the lncRNA's place (plain Gotoh, +5 / -4, every non-ACGT letter -4,
 * U read as A, gap 16 then 4, floored at 0, zero-score pad rows up to 16 * ceil(len / 16)); records are cut, numbered, sharded
 * (seg_first, seg_count) and same-letter segments skipped exactly as in fasim_scan_records_sites, and dna == NULL with nrec == 1,
 * rec_off == NULL and rec_len == NULL is the whole resident buffer.  out_sites[q * nrec + r] (wanted iff out_sites != NULL) is the
 * fasim_sites that section 14 defines for oligo q and record r under min_value and max_gap: it merges with fasim_sites_merge and
 * prints with fasim_sites_bed.  out_tracks[q * nrec + r] (wanted iff out_tracks != NULL) is the fasim_track of width `bin` of record r
 * scanned alone against oligo q: it merges with fasim_track_merge.  totals[q] (may be NULL): segments, skipped segments, units and
 * cells of oligo q; the kernel times of the call are shared evenly among the oligos.  No triplex records are made (no stage 3), the
 * engine's own query (fasim_set_query) is neither used nor changed, and the results depend on the oligo, the record and the
 * parameters only (not on the panel's order, batches, workers, shards, resident or streamed DNA).
 * Refusals, all before any GPU work, the engine stays usable: nq < 1, an empty oligo or one above FASIM_MAX_OLIGO nt (the message
 * names it and points to fasim_scan_records_sites), both outputs NULL, min_value outside [1, 16383] or max_gap < 0 when sites are
 * wanted, bin < 1 when tracks are wanted, and the record refusals of fasim_scan_records give FASIM_E_ARG; classicSim gives
 * FASIM_E_UNSUPPORTED. */
#define FASIM_MAX_OLIGO 112
int  fasim_scan_oligos(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                       const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                       int64_t seg_first, int64_t seg_count, const fasim_params* p,
                       int32_t min_value, int32_t max_gap, fasim_sites** out_sites /* [nq * nrec] or NULL */,
                       int32_t bin, fasim_track** out_tracks /* [nq * nrec] or NULL; bin >= 1 */,
                       fasim_scan_stats* totals /* [nq], may be NULL */);
/* The panel table `fasim --oligos --sites V` writes: the line of column names, then one tab-separated line per oligo in panel order:
 * oligo length total_sites covered_bases, then for ParaPlus ParaMinus AntiMinus AntiPlus each <Class>_sites <Class>_max.  sites is
 * [nq * nrec] as fasim_scan_oligos fills it; the counts and covered_bases (the sum of end - start) are sums over all records and, for
 * the first two, classes, <Class>_max the largest site value of the class over all records, 0 without a site (nrec == 0: all zeros).  Free with fasim_free. */
int  fasim_oligo_panel_tsv(const char* const* names, const int32_t* lens, int32_t nq, const fasim_sites* const* sites, int32_t nrec,
                           char** text, int64_t* text_len);
/* The sites of a panel and the hit of every site (csrc/site_short.hip): fasim_scan_oligos with sites wanted
 * (its arguments, refusals and totals; out_sites is byte for byte what it returns), then per oligo q and record r the hit list
 * out_hits[q * nrec + r] of out_sites[q * nrec + r]: section 15's definition with the oligo in the lncRNA's place.  The hit lists
 * are fasim_site_hits: they merge with fasim_site_hits_merge, print with fasim_site_hits_tsv and free with fasim_site_hits_free.
 * Every site of a call with cutLength above 6 000 keeps cigar_len = -1.  out_sites == NULL or out_hits == NULL: FASIM_E_ARG.  On
 * failure both outputs are freed and NULL; FASIM_E_NOMEM (no device memory for a chunk of the hits phase) leaves the engine usable.
 * Option site_short / FASIM_SITE_SHORT = 0 finds the end and start cells with k_site_ends instead of k_site_ends_short: the same
 * results, slower. */
int  fasim_scan_oligos_aligned(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                               const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                               int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t min_value, int32_t max_gap,
                               fasim_sites** out_sites /* [nq * nrec] */, fasim_site_hits** out_hits /* [nq * nrec] */,
                               fasim_scan_stats* totals /* [nq], may be NULL */);
/* The per-base profile of every oligo of a panel (csrc/scan_short.hip k_scan_short_rows, csrc/rowfold.hip k_rowfold_parts, DESIGN.md
 * section 24): fasim_scan_tfo_profile's R[c][i] with the oligo in the lncRNA's place -- the largest local alignment score that ends
 * on base i of the oligo, over the selected units of class c and their real columns, under the scoring of fasim_scan_oligos; the pad
 * rows are not part of the result.  out_profiles[q], or with per_record out_profiles[q * nrec + r] (what record r scanned alone
 * gives), are fasim_tfo_profile objects: they merge with fasim_tfo_profile_merge (shards: element-wise maximum), print with
 * fasim_tfo_profile_tsv and free with fasim_tfo_profile_free.  No value exceeds 5 * 112 = 560: saturated_units is 0.  Arguments,
 * totals and refusals as fasim_scan_oligos (without the sites' and tracks' own); out_profiles == NULL: FASIM_E_ARG. */
int  fasim_scan_oligos_profile(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                               const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                               int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t per_record,
                               fasim_tfo_profile** out_profiles /* [nq] or, per_record, [nq * nrec] */,
                               fasim_scan_stats* totals /* [nq], may be NULL */);
/* The screen of a panel (DESIGN.md section 12 with the oligo's potential): out_peaks[(q * nrec + r) * 4 + c] is the (value, pos, enc)
 * of fasim_scan_records_track for oligo q, record r and class c -- the largest potential, its first position, the smallest encoding
 * that attains it there, (0, -1, -1) where the potential is zero -- copied as 64 bytes per slice, not as tracks.  bin == 0: peaks only,
 * out_tracks must be NULL; bin >= 1: out_tracks[q * nrec + r] is fasim_scan_oligos' track as well.  Peaks of shards merge with
 * fasim_peaks_merge and print with fasim_screen_tsv.  Arguments, totals and refusals as fasim_scan_oligos (without the sites' own);
 * out_peaks == NULL, bin < 0, bin == 0 with out_tracks, bin >= 1 without: FASIM_E_ARG. */
int  fasim_scan_oligos_peaks(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                             const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                             int64_t seg_first, int64_t seg_count, const fasim_params* p, int32_t bin,
                             fasim_track** out_tracks /* [nq * nrec]; NULL with bin 0 */, fasim_peak* out_peaks /* [nq * nrec * 4] */,
                             fasim_scan_stats* totals /* [nq], may be NULL */);

/* ---- histograms of the potential with shuffled controls (csrc/hist.hip) -------------------------------------- */
/* How much of a record set reaches potential v, for every v.  P[c][x] is the bin = 1 track of section 11 of a record scanned alone.
 * n[c][v] is the number of COVERED positions x, over all records of the set, with P_r[c][x] == v, v in [0, 16383]; a position is
 * covered when a selected segment contains it (a segment that the same-letter rule skips is selected: its positions have P = 0).
 * The four classes sum to the same number, `positions`; for an unsharded call that is the total length of the records.  A position
 * in the overlap of two segments counts once, with the maximum of the two.  With a segment range, a boundary whose other segment
 * lies outside the range is PENDING: its positions are counted with the values of the range alone, and those values travel in
 * `pending` so that fasim_hist_merge can count the maximum of the two sides instead.  Boundary b of a record is the overlap of its
 * segments b and b + 1; side 0 holds the values of segment b (its last positions), side 1 those of segment b + 1 (its first). */
#define FASIM_HIST_BINS 16384
typedef struct fasim_hist_edge {
	int32_t record, side;                        /* record of the call's set; 0 / 1 as above                                */
	int64_t boundary;
	int32_t len, reserved;                       /* positions of the overlap                                                */
	uint16_t* v;                                 /* [4][len]: P of the range at those positions, per class                  */
} fasim_hist_edge;
typedef struct fasim_hist {
	int64_t* n[FASIM_TRACK_CLASSES];             /* [FASIM_HIST_BINS]                                                       */
	int64_t positions;                           /* covered positions = the sum of n[c][.] for every c                      */
	int64_t units, saturated_units;              /* as fasim_track                                                          */
	int64_t npending; fasim_hist_edge* pending;  /* ordered by (record, boundary, side)                                     */
} fasim_hist;
/* fasim_scan_records with one histogram per query over the whole record set: arguments, record cutting, global segment numbering
 * and the refusals of fasim_scan_records_sites (without min_value and max_gap); out_hists == NULL gives FASIM_E_ARG, and
 * 2 * overlapLength > cutLength gives FASIM_E_UNSUPPORTED (a base would lie in three segments).  Every refusal happens before any
 * GPU work and leaves the engine usable, as does FASIM_E_NOMEM.  out_results == NULL: no stage 3 (the work ends after the scan
 * kernel and k_hist); otherwise out_results and totals are byte for byte those of fasim_scan_records.  out_hists[q] depends on the
 * records, the query and the parameters only (not on batches, workers, shards after the merge, devices, dp_f16, resident or streamed
 * DNA, nor on whether stage 3 ran).  A control is just one more query: see fasim_shuffle_query.  Free each with fasim_hist_free. */
int  fasim_scan_records_hist(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                             const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                             int64_t seg_first, int64_t seg_count, const fasim_params* p,
                             fasim_result** out_results /* [nq * nrec] or NULL: no stage 3 */,
                             fasim_hist** out_hists /* [nq] */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* The same for a panel of oligos: the arguments and refusals of fasim_scan_oligos (without the sites' and tracks' own), plus the
 * 2 * overlapLength > cutLength refusal; out_hists[q] is the histogram of oligo q over the record set. */
int  fasim_scan_oligos_hist(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                            const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                            int64_t seg_first, int64_t seg_count, const fasim_params* p,
                            fasim_hist** out_hists /* [nq] */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* Shards of ONE record set and one query (disjoint segment ranges): counts, positions, units and saturated_units are summed; where
 * both sides of a boundary are pending, what each side counted alone is taken out, the element-wise maximum is counted once and the
 * pair is dropped; unpaired edges stay pending.  Associative and commutative; the merge of all shards is the unsharded result with
 * nothing pending.  An edge that is pending twice, or two sides of different length, are refused (FASIM_E_ARG). */
int  fasim_hist_merge(const fasim_hist* const* parts, int32_t nparts, fasim_hist** out);
void fasim_hist_free(fasim_hist* h);
/* Control k (k >= 1) of a query under `seed`: a Fisher-Yates shuffle of the m bytes as given (case and U kept), driven by a
 * splitmix64 whose state starts at seed ^ (k * 0xD1B54A32D192ED03) mod 2^64: for i = m - 1 down to 1, j = next() mod (i + 1), swap
 * a[i] and a[j].  out[m] may be rna itself.  The shuffle keeps the composition exactly. */
int  fasim_shuffle_query(const char* rna, int32_t m, uint64_t seed, int32_t k, char* out /* [m] */);
/* With ge[v] = the sum over the classes of n[c][w], w >= v, and ctl_ge[v] the same summed over the K controls: the smallest v >= 1
 * with ge[v] > 0 such that every w >= v with ge[w] > 0 has (double)ctl_ge[w] <= Q * (double)K * (double)ge[w]; 0 when there is none.
 * K is ncontrols and Q is fdr.  Bad arguments (K < 0, Q outside (0, 1]) give FASIM_E_ARG (negative). */
int32_t fasim_hist_threshold(const fasim_hist* real, const fasim_hist* const* controls, int32_t ncontrols, double fdr);
/* The table `fasim --potential-hist` writes.  First `# fasim potential histogram lncRNA=<rna_name> positions=<n>` and, with K > 0,
 * ` controls=<K> seed=<S> fdr=<Q> min_value=<V|NA>` (V = fasim_hist_threshold, NA for 0; Q as %g).  Then the line of column names
 * and one tab-separated line per value v from 1 to the largest v with a count in the query or a control: value, per class <Class>
 * (n[c][v]), <Class>_ge and with K > 0 <Class>_ctl_ge, then all_ge and with K > 0 all_ctl_ge and fdr = all_ctl_ge / (K * all_ge) as
 * %.6g, NA where all_ge is 0 (K is ncontrols, S is seed, Q is fdr).  Free with fasim_free. */
int  fasim_hist_tsv(const fasim_hist* real, const fasim_hist* const* controls, int32_t ncontrols, uint64_t seed, double fdr, const char* rna_name,
                    char** text, int64_t* text_len);

/* ---- sites per threshold, with dinucleotide controls (csrc/hist_pairs.hip) --------------------------------- */
/* How many sites a record set has at every threshold.  Beside fasim_hist's n[c][v], pairs[c][w] is the number of pairs (x - 1, x) of
 * neighbouring covered positions of ONE record with min(P_r[c][x - 1], P_r[c][x]) == w, w in [0, 16383]; pairs never span two
 * records.  The number of maximal runs of positions with P >= v, which is the number of class-c sites that fasim_scan_records_sites
 * reports over the set with min_value v and max_gap 0, is
 *     sites[c][v] = the sum over w >= v of (n[c][w] - pairs[c][w]),   v >= 1,
 * since the runs of a threshold number its positions minus its adjacent pairs.  It is not monotone in v (a site can split as v
 * rises), hence two histograms.  `npairs` is the sum of pairs[c][.] for every c; for an unsharded call that is the total length of
 * the records minus their number.  Overlaps, skipped segments, saturation, units and the meaning of PENDING are fasim_hist's.  A
 * pending edge carries, beside the zone values, `nb`: the values of the range at the position next to the zone on the side of the
 * segment's interior (before the zone for side 0, after it for side 1), and `link`: 0 there is no such position (the record ends
 * with the zone), 1 it lies in one segment only, 2 it is the first (last) position of the segment's other zone, whose values change
 * when that boundary is merged (2 * overlapLength == cutLength only).  A zone of length 0 (overlapLength 0) still has its two nb. */
typedef struct fasim_site_counts_edge {
	int32_t record, side;                        /* as fasim_hist_edge                                                      */
	int64_t boundary;
	int32_t len, link;
	uint16_t nb[FASIM_TRACK_CLASSES];
	uint16_t* v;                                 /* [4][len]                                                                */
} fasim_site_counts_edge;
typedef struct fasim_site_counts {
	int64_t* n[FASIM_TRACK_CLASSES];             /* [FASIM_HIST_BINS]: fasim_hist's                                         */
	int64_t* pairs[FASIM_TRACK_CLASSES];         /* [FASIM_HIST_BINS]                                                       */
	int64_t positions, npairs;
	int64_t units, saturated_units;              /* as fasim_track                                                          */
	int64_t npending; fasim_site_counts_edge* pending;   /* ordered by (record, boundary, side)                             */
} fasim_site_counts;
/* fasim_scan_records_hist with site counts in the place of the histograms: the same arguments and refusals (out_counts == NULL:
 * FASIM_E_ARG; 2 * overlapLength > cutLength: FASIM_E_UNSUPPORTED; queries below 113 nt), the same meaning of out_results and
 * totals, the same independence of batches, workers, shards after the merge, dp_f16 and resident or streamed DNA.  n[][] is what
 * fasim_scan_records_hist counts.  Free each with fasim_site_counts_free. */
int  fasim_scan_records_site_counts(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                                    const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                                    int64_t seg_first, int64_t seg_count, const fasim_params* p,
                                    fasim_result** out_results /* [nq * nrec] or NULL: no stage 3 */,
                                    fasim_site_counts** out_counts /* [nq] */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* The same for a panel of oligos: the arguments and refusals of fasim_scan_oligos_hist. */
int  fasim_scan_oligos_site_counts(fasim_engine* e, const char* const* oligos, const int32_t* lens, int32_t nq,
                                   const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                                   int64_t seg_first, int64_t seg_count, const fasim_params* p,
                                   fasim_site_counts** out_counts /* [nq] */, fasim_scan_stats* totals /* [nq], may be NULL */);
/* Shards of ONE record set and one query (disjoint segment ranges), as fasim_hist_merge: everything is summed; where both sides of a
 * boundary are pending, the positions of the zone and the pairs of the chain nb(side 0), zone, nb(side 1) that each side counted
 * alone are taken out and those of the element-wise maximum are counted instead, the pair that straddles the far border of the zone
 * included.  Unpaired edges stay pending.  Associative and commutative; the merge of all shards is the unsharded result with
 * nothing pending.  An edge that is pending twice, or two sides of different length, are refused (FASIM_E_ARG). */
int  fasim_site_counts_merge(const fasim_site_counts* const* parts, int32_t nparts, fasim_site_counts** out);
void fasim_site_counts_free(fasim_site_counts* s);
/* Control k (k >= 1) of a query under `seed` that keeps every dinucleotide count, the first and the last byte (Altschul-Erickson):
 * a random Euler path through the graph of the query's bytes as given (case and U kept).  The splitmix64 state starts as in
 * fasim_shuffle_query.  m < 3 returns a copy.  Otherwise, with z = rna[m - 1]: (1) for each distinct byte value a in ascending
 * order, the list of the successors of a in order of occurrence; (2) for each a != z with a non-empty list, in ascending order, a
 * last edge j = next() mod len; (3) if following the last edges from every such a does not reach z, all of them are drawn again;
 * (4) each chosen last edge moves to the end of its list (the entries behind it move up by one) and the len' entries before it are
 * shuffled by fasim_shuffle_query's loop (for i = len' - 1 down to 1: j = next() mod (i + 1), swap), in ascending order of a; z's
 * whole list is shuffled; (5) the walk from rna[0] consumes each list in order.  out[m] may be rna itself. */
int  fasim_shuffle_query_dinuc(const char* rna, int32_t m, uint64_t seed, int32_t k, char* out /* [m] */);
/* fasim_hist_threshold on sites: with s[v] = the sum over the classes of sites[c][v] and ctl_s[v] the same summed over the K
 * controls, the smallest v >= 1 with s[v] > 0 such that every w >= v with s[w] > 0 has (double)ctl_s[w] <= Q * K * (double)s[w];
 * 0 when there is none.  Bad arguments give FASIM_E_ARG (negative). */
int32_t fasim_site_counts_threshold(const fasim_site_counts* real, const fasim_site_counts* const* controls, int32_t ncontrols, double fdr);
/* The table `fasim --potential-hist --hist-sites` writes.  First `# fasim site counts lncRNA=<rna_name> positions=<n>` and, with
 * K > 0, ` controls=<K> seed=<S> shuffle=<mono|di> fdr=<Q> min_value=<V|NA>` (V = fasim_site_counts_threshold; dinuc != 0: di).
 * Then the column names and one tab-separated line per value v from 1 to the largest v with a site in the query or a control:
 * value, per class <Class>_sites and with K > 0 <Class>_ctl_sites, then all_sites and with K > 0 all_ctl_sites and
 * fdr = all_ctl_sites / (K * all_sites) as %.6g, NA where all_sites is 0.  Free with fasim_free. */
int  fasim_site_counts_tsv(const fasim_site_counts* real, const fasim_site_counts* const* controls, int32_t ncontrols, uint64_t seed,
                           int32_t dinuc, double fdr, const char* rna_name, char** text, int64_t* text_len);

/* Host half of the path's one exchange step: concatenates the records of `nparts` shards in the
 * order given and rebases their pool offsets.  Shards are contiguous segment ranges, so rank order IS the
 * reference's canonical (segment, encoding, fastSIM rank) order, which cluster_triplex()'s unstable sort needs.
 * The result owns its memory (fasim_result_free); stats are zero. */
int fasim_merge_results(const fasim_triplex* const* recs, const int64_t* counts, const char* const* pools,
                        const int64_t* pool_lens, int32_t nparts, fasim_result** out);
/* In-place form for a gather that receives every shard's records and pool directly at their final positions of one
 * flat buffer (what gather_results() of the Python package does over RCCL): adds `delta` (= the bytes of pool that
 * precede this shard's pool) to the pool offsets of `count` records. */
int fasim_rebase_offsets(fasim_triplex* recs, int64_t count, int64_t delta);
/* Optional: upload a DNA record once and keep it resident in HBM (and a host copy for the string work);
 * afterwards fasim_scan(e, NULL, 0, ...) scans the resident record without any H2D copy of the sequence, and
 * fasim_scan_records(e, ..., NULL, offsets, lengths, ...) the records of a resident set (which may exceed 2^31 nt). */
int fasim_load_dna(fasim_engine* e, const char* dna, int64_t dna_len);
void fasim_result_free(fasim_result* r);
int64_t fasim_segment_count(int64_t dna_len, const fasim_params* p);   /* cutSequence(): fastsim.h:71 */

/* ---- host tail: main() coordinates + cluster_triplex() + printResult() ------------------------- */
/* (Fasim-LongTarget.cpp:141-149, 600-691, 797-829).  Takes the concatenation of all shards' records
 * in canonical order and returns the bytes of the -TFOsorted file (malloc'd; free with fasim_free).  */
int fasim_tfosorted(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len,
                    const char* chr, int64_t start_genome, const fasim_params* p,
                    char** text, int64_t* text_len);
/* print_cluster() (Fasim-LongTarget.cpp:694-795): the bytes of the -TFOclass<level>-<ds>-<lg> bedGraph file for
 * class `level` (the reference writes levels 1 and 2, :832).  Clusters the records itself; dna_len = record length. */
int fasim_tfoclass(const fasim_triplex* recs, int64_t count, int32_t level, const char* chr, int64_t start_genome,
                   int64_t dna_len, const char* rna_name, const fasim_params* p, char** text, int64_t* text_len);
/* The same two with a flags word.  FASIM_TAIL_CLAMP_CLUSTER: when a triplex mid-point lies within -ds of the query
 * start, cluster_triplex() of the reference indexes std::map<size_t,...> with a negative number and never terminates
 * (Fasim-LongTarget.cpp:641-688; needs -lg below about 2*-ds).  Without the flag such input is refused
 * (FASIM_E_UNSUPPORTED); with it the positions before the query start are treated as non-existent, which is what the
 * reference's arithmetic means and gives a defined, terminating result (identical to the reference wherever the
 * reference terminates). */
#define FASIM_TAIL_CLAMP_CLUSTER 1
int fasim_tfosorted_ex(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len,
                       const char* chr, int64_t start_genome, const fasim_params* p, int32_t flags,
                       char** text, int64_t* text_len);
int fasim_tfoclass_ex(const fasim_triplex* recs, int64_t count, int32_t level, const char* chr, int64_t start_genome,
                      int64_t dna_len, const char* rna_name, const fasim_params* p, int32_t flags,
                      char** text, int64_t* text_len);
/* printResult() as a whole (Fasim-LongTarget.cpp:797-836): the -TFOsorted text and the two -TFOclass texts (levels 1 and 2)
 * from ONE clustering of the records (the separate calls above each cluster again).  Free each text with fasim_free. */
int fasim_tail_outputs(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len, const char* chr,
                       int64_t start_genome, int64_t dna_len, const char* rna_name, const fasim_params* p, int32_t flags,
                       char** tfosorted, int64_t* tfosorted_len, char** class1, int64_t* class1_len,
                       char** class2, int64_t* class2_len);
void fasim_free(void* p);
/* ---- BED intervals (`fasim --regions`, read_bed() of the Python package) --------------------------------------------- */
/* One interval of a BED file: 0-based, half-open [start, end) on `chrom`; line = its 1-based line in the file.  name = column 4,
 * else "<chrom>_<start+1>_<end>"; an interval whose (name, chrom) pair an earlier one already has gets "_<line>" appended
 * (repeatedly if need be), so that every interval's output stem <name>-<lnc>-<f1 stem>.<chrom> is unique. */
typedef struct fasim_region {
	int64_t line, start, end;
	const char* chrom;                  /* strings live in the same block as the array */
	const char* name;
} fasim_region;
/* BED3 ... BED6 and wider, whitespace-separated; columns after the 4th are ignored (the strand too: the scan covers both strands
 * through its 48 encodings).  Blank lines, '#' lines and "track" / "browser" lines are skipped.  Refused with FASIM_E_ARG (the
 * line number and the reason in fasim_last_error(NULL)): fewer than 3 columns, a start or end that is not an integer,
 * start < 0, end <= start, end - start > 2^31 - 1, an unreadable file.  *out is ONE block (free it with fasim_free); *n may be 0. */
int fasim_read_bed(const char* path, fasim_region** out, int64_t* n);
/* The bytes of `fasim --screen`'s table for n intervals: a header line, then one line per interval in the order given, columns
 * line name chrom start end segments and, per class in order (ParaPlus ParaMinus AntiMinus AntiPlus), <Class> <Class>_pos
 * <Class>_rule: the peak value, its 0-based genome coordinate regions[k].start + pos, and the Rule value -TFOsorted prints for the
 * peak's encoding.  A zero peak has NA in its _pos and _rule columns; an interval with segments[k] < 0 (not scanned: it lies in no
 * DNA record) has NA in every column after `end`.  peaks: [n * 4], positions relative to the interval.  Free with fasim_free. */
int fasim_screen_tsv(const fasim_region* regions, const int64_t* segments, const fasim_peak* peaks, int64_t n,
                     char** text, int64_t* text_len);
/* ---- variants scored by the triplex potential through them (csrc/variant.hip) ------------------------------- */
/* Does a variant make or break a triplex site?  Per variant, allele (0 = REF, 1 = ALT) and strand class: the best score of a local
 * alignment of the query that passes through the allele, in the allele's window of the record.  With flank F the window of a variant
 * at record offset pos is record[lo, hi), lo = max(0, pos - F), hi = min(record length, pos + ref_len + F), with the allele in the
 * place of REF; its own columns are the mark.  Scoring is that of section 11 (plain Gotoh, +5 / -4 over ACGT, every other letter -4,
 * U read as A, gap 16 then 4, the units of fasim_encode_unit, enabled encodings and classes as everywhere) with three differences:
 * no pad rows, no same-letter skip, no saturation (int32 values; a window has at most 5 120 columns).  The touching matrix T is the
 * plain local recurrence in the columns before the mark's end and from there on the same with a diagonal term that only continues
 * (Hdiag > 0 ? Hdiag + s : 0); the value of a unit is the maximum of T over the columns from the mark's first on.  value[a][c] is the
 * maximum over the class's enabled encodings, enc[a][c] the smallest encoding that attains it (-1: value 0).  flags bit 0, `clipped`:
 * an alignment of the largest value over both alleles and all classes may continue past an end of the window that the flank cut (not
 * the record's end): lengthen the flank. */
#define FASIM_MAX_ALLELE 1024
#define FASIM_MAX_FLANK  2048
typedef struct fasim_variant {
	int64_t line, pos;                  /* 1-based line of the VCF; 0-based offset of REF's first letter within record `rec`       */
	int32_t rec, ref_len, alt_len;      /* alt_len < 0: an allele that cannot be scored (the entry gets zeros and enc = -1)         */
	const char* chrom; const char* id; const char* ref; const char* alt;      /* strings live in the same block as the array */
} fasim_variant;
typedef struct fasim_variant_score {
	int32_t value[2][FASIM_TRACK_CLASSES], enc[2][FASIM_TRACK_CLASSES];
	int32_t flags, reserved;
} fasim_variant_score;
typedef struct fasim_variant_stats { int64_t problems, cells; double kernel_s, total_s; } fasim_variant_stats;
/* VCF text, tab-separated: CHROM POS ID REF ALT, further columns ignored, '#' lines and blank lines skipped.  An ALT with commas
 * gives one entry per allele with the same `line`; alleles are upper-cased; pos = POS - 1 and rec = 0.  Kept with alt_len = -1 (the
 * caller reports NA): a symbolic allele (<DEL>), a `*` or `.` allele, a breakend, an allele with letters outside ACGTN or longer
 * than FASIM_MAX_ALLELE.  Refused with FASIM_E_ARG (the line number and the reason in fasim_last_error(NULL)): fewer than 5 columns,
 * a POS that is not an integer or below 1, an empty REF or ALT, an unreadable file.  *out is ONE block (fasim_free); *n may be 0. */
int fasim_read_vcf(const char* path, fasim_variant** out, int64_t* n);
/* Scores nvar variants of the records dna[rec_off[r] .. rec_off[r] + rec_len[r]) (dna == NULL: the resident buffer of fasim_load_dna)
 * for nq >= 1 queries; out[q * nvar + v].  The engine's own query (fasim_set_query), its scan buffers and its workers are neither read
 * nor changed.  The result of a variant depends on the record, the variant, the flank, the query and the parameters only (not on the
 * other variants, their order or the launches).  REF is not compared with the record: that is the caller's business.  Refused before
 * any GPU work, the engine stays usable: a variant outside its record, ref_len < 1, an allele above FASIM_MAX_ALLELE or of length 0,
 * a flank outside [0, FASIM_MAX_FLANK], the record refusals of fasim_scan_records (FASIM_E_ARG); a query above FASIM_MAX_QUERY,
 * classicSim (FASIM_E_UNSUPPORTED). */
int fasim_score_variants(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                         const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                         const fasim_variant* vars, int64_t nvar, int32_t flank, const fasim_params* p,
                         fasim_variant_score* out /* [nq * nvar] */, fasim_variant_stats* stats /* may be NULL */);
/* The table `fasim --variants` writes for one query: `# fasim variants lncRNA=<rna_name> flank=<F>`, the line of column names, then
 * one tab-separated line per entry: line chrom pos id ref alt, per class <Class>_ref <Class>_alt, then max_ref max_alt delta
 * rule_ref rule_alt clipped.  pos is 1-based as in the VCF; delta = max_alt - max_ref; rule_* is the Rule value -TFOsorted prints for
 * the smallest class, then the smallest encoding, that attains the maximum, NA where it is 0.  An entry with matched[k] == 0
 * (matched may be NULL: all matched) or alt_len < 0 has NA in every column after alt.  Free with fasim_free. */
int fasim_variants_tsv(const fasim_variant* vars, const fasim_variant_score* scores, int64_t nvar, int32_t flank, const char* rna_name,
                       const uint8_t* matched /* [nvar] or NULL */, char** text, int64_t* text_len);
/* ---- the alignment behind every variant score (csrc/variant_path.hip) ---------------------------------------- */
/* The HIT of a slot (variant, allele, class) with value > 0 is the alignment the touching matrix T counted, in the unit of the
 * encoding fasim_score_variants reports for the slot.  End cell (i1, j1): the smallest column j1 >= v0 at which a real row holds
 * T == value, the smallest such row i1.  Path: traced back in T from (i1, j1) in state H with fixed priorities -- with d the diagonal
 * neighbour's T (0 outside the matrix) and s the pair's score: d > 0 and T == d + s: diagonal; else d == 0, j < v1 and T == s: the
 * alignment's first pair (i0, j0), stop; else T == E: state E; else state F; in a gap state extend before open.  E consumes a target
 * column (CIGAR D), F a query row (CIGAR I).  The CIGAR begins with M; it ends with M, or with one D run where the allele is reached
 * only through a gap.  The record is that of section 15: the alignment goes through the conversion of fasim_scan with -ni 1 and no
 * -na over the window's letters (the ALT window for allele 1), dna_start = the window's first record offset, t.seg = the variant's
 * index in the call, t.score = value.
 * fasim_variant_window: the letters of the record before (pre) and after (post) REF inside the flank; edge bit 0 / 1: the lower /
 * upper end of the window was cut by the flank and not by the record's end. */
typedef struct fasim_variant_window { int32_t pre, post, edge, reserved; } fasim_variant_window;
/* fasim_score_variants and the hit of every slot: the arguments, refusals and -- byte for byte -- the scores of fasim_score_variants,
 * then windows[v] and hits[q] (both required, else FASIM_E_ARG): hits[q]->n = 8 * nvar, hit (v * 2 + allele) * 4 + class; q_begin,
 * q_end, t_begin, t_end = i0, i1, j0, j1 in the unit.  A slot without a value has cigar_len 0, nt 0, cells -1 and empty strings.  A
 * slot whose problem has more than 2^26 cells (query length x window length), or whose path the kernel did not find, has
 * cigar_len -1 and is counted in `unaligned`.  Hits are never filtered.  The hit depends on the record, the variant, the flank, the
 * query and the parameters only.  FASIM_E_NOMEM leaves the engine usable.  Free each hits[q] with fasim_site_hits_free. */
int fasim_score_variants_aligned(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                                 const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                                 const fasim_variant* vars, int64_t nvar, int32_t flank, const fasim_params* p,
                                 fasim_variant_score* out /* [nq * nvar] */, fasim_variant_stats* stats /* may be NULL */,
                                 fasim_variant_window* windows /* [nvar] */, fasim_site_hits** hits /* [nq] */);
/* Pure host code: the reference bases [*start, *end) (0-based, in the coordinates of v->pos) that the unit columns [j0, j1] of a hit
 * of `allele` under `enc` cover.  The columns are window letters [w0, w1] in forward orientation (w = n - 1 - j for an odd
 * encoding); letters before the allele map to themselves, letters of the allele to REF's range (start: its first base, end: its
 * last), letters behind it are shifted by the difference of the alleles' lengths.  For allele 0 this is the identity.  *clipped
 * (may be NULL): the columns include the unit's first column and that end of the window was cut by the flank, or its last column
 * and that end was cut.  FASIM_E_ARG: a NULL pointer, an allele outside {0, 1}, an encoding outside [0, 48), columns outside the
 * window. */
int fasim_variant_hit_span(const fasim_variant* v, const fasim_variant_window* w, int32_t allele, int32_t enc, int32_t j0, int32_t j1,
                           int64_t* start, int64_t* end, int32_t* clipped);
/* The table `fasim --variants --variant-hits` writes for one query: `# fasim variant hits lncRNA=<rna_name> flank=<F>`, the line of
 * column names, then one tab-separated line per (entry, allele, class) with value > 0, ref before alt, classes in their order: line
 * chrom pos id ref alt allele class value rule strand tts_start tts_end tfo_start tfo_end nt identity stability cigar clipped TFO
 * TTS.  tts_start / tts_end: fasim_variant_hit_span; tfo_start / tfo_end: 1-based inclusive query positions; rule, strand, identity,
 * stability and cigar as fasim_site_hits_tsv prints them.  An unaligned hit has NA from tts_start on.  An entry with matched[k] == 0
 * or alt_len < 0 gets no lines.  hits->n must be 8 * nvar.  Free with fasim_free. */
int fasim_variant_hits_tsv(const fasim_variant* vars, const fasim_variant_score* scores, const fasim_variant_window* windows,
                           const fasim_site_hits* hits, int64_t nvar, int32_t flank, const char* rna_name,
                           const uint8_t* matched /* [nvar] or NULL */, char** text, int64_t* text_len);
/* ---- variants scored on a sample's phased haplotypes (csrc/haplotype.hip) ----------------------------------- */
/* fasim_score_variants exchanges REF for ALT in a window of reference letters; a person carries the window with their other variants
 * in it.  Entries are those of fasim_read_vcf; a genotype per entry says which haplotype of one sample carries its ALT:
 * hap[h] 1 = this ALT, 0 = REF or another ALT of the line, -1 = missing (`.`); phased 1 = the GT separator is `|`, or the call is
 * haploid (which counts as both haplotypes alike).
 * The consistent set A_h of haplotype h in a record: over the record's entries in the order (pos, line, entry index), an entry
 * qualifies with alt_len >= 0, matched, hap[h] == 1 and (phased or hap[0] == hap[1] == 1), and a qualifying entry is accepted iff its
 * REF span [pos, pos + ref_len) intersects no accepted span (touching spans do not intersect).  The applied neighbours of a focus
 * entry v are A_h without the entries of v's own line and without entries whose REF span intersects v's.  R_h(v) is the record with
 * every applied neighbour's REF span replaced by its ALT, a' = v.pos plus the sum of alt_len - ref_len over the applied neighbours
 * before v.  The result of (v, h) is what fasim_score_variants defines for the variant (a', ref_len, alt) on the record R_h(v) with
 * the same flank: window, mark, values, encodings and clip bit; the flank counts letters of the haplotype, R_h's ends are the
 * record's ends.  Where nothing is applied it is today's score byte for byte. */
typedef struct fasim_genotype { int8_t hap[2]; uint8_t phased, pad; } fasim_genotype;
/* carried[h]: 1 = this ALT, 0 = REF, 2 = another ALT of the line, -1 = missing.  applied[h]: the applied neighbours with at least one
 * letter in the windows.  flags[h]: bit 0 the clip bit of fasim_variant_score over both alleles on this haplotype; bit 1 an entry of
 * another line within |pos - v.pos| <= flank + FASIM_MAX_ALLELE has hap[h] == 1 but is an unphased heterozygote (it was not applied;
 * an entry that is unmatched or cannot be scored is never applied and sets no bit);
 * bit 2 an entry of another line within the same distance qualified but was rejected for overlap (with A_h, or with the focus); bit 3
 * the windows of haplotype 1 equal those of haplotype 0 letter for letter, so they were computed once (set on both). */
typedef struct fasim_hap_score { fasim_variant_score hap[2]; int32_t carried[2], applied[2], flags[2]; } fasim_hap_score;
/* fasim_read_vcf with the genotypes of one sample: the same entries in the same order, (*gts)[k] the genotype of entry k (a block of
 * its own: fasim_free).  GT is found through the FORMAT column (the 9th), the sample by its name in the #CHROM line.  Refused with
 * FASIM_E_ARG and the reason, besides fasim_read_vcf's refusals: a sample the #CHROM line does not name (or no #CHROM line before
 * the first data line), a data line without the sample's column, no GT in FORMAT, a malformed GT (an allele that is neither `.` nor
 * an index of the line's alleles, more than two alleles). */
int fasim_read_vcf_sample(const char* path, const char* sample, fasim_variant** out, int64_t* n, fasim_genotype** gts);
/* Pure host code: the window of entry v on haplotype hap (0 / 1) for `allele` (0 REF, 1 ALT) in haplotype letters, as the planner of
 * fasim_score_haplotypes builds it from pieces.  Only the entries of v's record (vars[k].rec == vars[v].rec) are looked at;
 * `record` are that record's rec_len letters.  *letters (fasim_free) holds *n letters, the allele's are [*v0, *v0 + allele length);
 * *edge bit 0 / 1: the lower / upper end was cut by the flank and not by the haplotype's end. */
int fasim_haplotype_window(const fasim_variant* vars, const fasim_genotype* gts, int64_t nvar, const uint8_t* matched /* or NULL */,
                           int64_t rec_len, const char* record, int64_t v, int32_t hap, int32_t allele, int32_t flank,
                           char** letters, int32_t* n, int32_t* v0, int32_t* edge);
/* Pure host code: what the planner decides for entry v before any score exists: carried[2], applied[2] and flags[2] of
 * fasim_hap_score, flags without bit 0. */
int fasim_haplotype_info(const fasim_variant* vars, const fasim_genotype* gts, int64_t nvar, const uint8_t* matched /* or NULL */,
                         int64_t rec_len, const char* record, int64_t v, int32_t flank, int32_t* carried, int32_t* applied, int32_t* flags);
/* Scores every entry on both haplotypes: out[q * nvar + v].  Arguments and refusals as fasim_score_variants; matched[k] == 0 (NULL:
 * all matched) keeps entry k from being applied as a neighbour (it is still scored).  A haplotype without an applied neighbour in
 * reach takes the plain windows of fasim_score_variants; two haplotypes with equal windows are computed once.  The result of (v, h)
 * depends on the record, the entries with their genotypes, the flank, the query and the parameters only.  stats: both parts added. */
int fasim_score_haplotypes(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                           const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                           const fasim_variant* vars, const fasim_genotype* gts, const uint8_t* matched /* [nvar] or NULL */, int64_t nvar,
                           int32_t flank, const fasim_params* p, fasim_hap_score* out /* [nq * nvar] */, fasim_variant_stats* stats /* may be NULL */);
/* The table `fasim --variants --sample` writes for one query: `# fasim haplotypes lncRNA=<rna_name> sample=<sample> flank=<F>`, the
 * line of column names, then one line per entry: line chrom pos id ref alt gt, then for h1 and h2: carried applied, per class
 * <Class>_ref <Class>_alt, max_ref max_alt delta rule_ref rule_alt value, flags; then diplotype_max.  gt is the entry's own genotype
 * (1 = this ALT, 0 = not, . = missing; `|` phased, `/` not).  value is the maximum of the allele the haplotype carries (max_alt for
 * carried 1, max_ref for carried 0), NA for carried 2 or -1; diplotype_max the larger of the two values, NA unless both are numbers.
 * An entry with matched[k] == 0 or alt_len < 0 has NA in every column after gt.  Free with fasim_free. */
int fasim_haplotypes_tsv(const fasim_variant* vars, const fasim_genotype* gts, const fasim_hap_score* scores, int64_t nvar, int32_t flank,
                         const char* rna_name, const char* sample, const uint8_t* matched /* [nvar] or NULL */, char** text, int64_t* text_len);
/* ---- every SNV of an interval from one shared pass (csrc/mutagenesis.hip) ------------------------------------- */
/* Which bases of an interval matter?  An interval is [start, end) of record `rec`, 0-based, at least one base.  With flank F its
 * context is C = record[lo, hi), lo = max(0, start - F), hi = min(record length, end + F).  For a position x of the interval and a
 * letter b of ACGT, C(x, b) is C with byte x - lo replaced by the upper-case byte b, and the result of (x, b) under an encoding is
 * what fasim_score_variants defines for the window C(x, b) with the mark [x - lo, x - lo + 1) and the edges (lo > 0, hi < record
 * length): scoring, touching matrix, 2 * value + clip bit and the reduction over classes and encodings are section 19's word for
 * word.  All positions of an interval share the one context, where fasim_score_variants gives every variant a flank of its own:
 * the window [start - F, end + F) is never smaller than the SNV's own [x - F, x + 1 + F), so a value here is never below
 * fasim_score_variants' value for the same SNV and flank.
 * value[b][c], enc[b][c]: letter b, strand class c (enc -1: value 0).  ref: the index in ACGT of the record's byte at x if it is
 * one of those four upper-case bytes, else -1 (all four letters are still scored).  clipped[b]: bit 0 of the largest 2 * value + bit
 * of letter b over all classes and encodings; the clip flag of the SNV ref -> b is the bit of the larger of the two letters' words
 * 2 * max value + clipped (ties go to the bit). */
typedef struct fasim_interval { int32_t rec, reserved; int64_t start, end; } fasim_interval;
typedef struct fasim_mut_score {
	int32_t value[4][FASIM_TRACK_CLASSES];
	int8_t enc[4][FASIM_TRACK_CLASSES];
	int8_t ref; uint8_t clipped[4]; uint8_t reserved[3];
} fasim_mut_score;
/* prefix_problems: (context, encoding, position range) runs of the shared pass and the columns they ran; problems: (position,
 * letter, encoding) continuations and the columns they ran until their dead column; cont_cols_bound: what cont_cols would be with no
 * early stop, the sum of n - c over the problems; prefix_s, cont_s: HIP-event seconds of k_mut_prefix and k_mut_touch. */
typedef struct fasim_mutagenesis_stats {
	int64_t intervals, positions, prefix_problems, problems, launches, prefix_cols, cont_cols, cont_cols_bound;
	double prefix_s, cont_s, total_s;
} fasim_mutagenesis_stats;
/* Scores every position of nint intervals for nq >= 1 queries (1 to FASIM_MAX_QUERY nt): out[q * npos + k], npos the sum of the
 * intervals' lengths, the positions in interval order and ascending within an interval.  Records, engine state and stream as
 * fasim_score_variants.  The result of a position depends on the record, the interval, the flank, the query and the parameters only
 * (not on the other intervals, their order or the launches).  Refused before any GPU work, the engine stays usable: an interval
 * outside its record or with end <= start, (end - start) + 2 * flank > 5120, a flank outside [0, FASIM_MAX_FLANK], the record
 * refusals of fasim_score_variants (FASIM_E_ARG); a query above FASIM_MAX_QUERY, classicSim (FASIM_E_UNSUPPORTED). */
int fasim_score_mutagenesis(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                            const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                            const fasim_interval* intervals, int64_t nint, int32_t flank, const fasim_params* p,
                            fasim_mut_score* out /* [nq * npos] */, fasim_mutagenesis_stats* stats /* may be NULL */);
/* The table `fasim --mutagenesis` writes for one query: `# fasim mutagenesis lncRNA=<rna_name> flank=<F>`, the column names of
 * fasim_variants_tsv, then one line per (position, letter other than the reference letter, in ACGT order), positions ascending,
 * intervals in the order given: line = regions[k].line, chrom, pos 1-based, id = regions[k].name, ref, alt, per class
 * <Class>_ref <Class>_alt, max_ref max_alt delta rule_ref rule_alt clipped as fasim_variants_tsv prints them.  scores: the positions
 * of interval k are scores[offsets[k] .. offsets[k + 1]) (an interval that was not scored has none); a position with ref == -1 gets
 * no lines.  Free with fasim_free. */
int fasim_mutagenesis_tsv(const fasim_region* regions, const int64_t* offsets /* [n + 1] */, int64_t n, const fasim_mut_score* scores,
                          int32_t flank, const char* rna_name, char** text, int64_t* text_len);
/* ---- every deletion of an interval from the same shared pass (csrc/mutagenesis.hip) --------------------------- */
/* Which deletions inside an interval matter?  Interval, flank, context C = record[lo, hi) and the bound (end - start) + 2 * flank <=
 * 5120 are section 26's.  lengths: 1 to FASIM_MAX_DELETION_LENGTHS strictly ascending integers in [1, FASIM_MAX_ALLELE - 1].  A
 * deletion is (x, d), d one of the lengths, x in [start, end), x + d < end: base x, the anchor of a VCF line, stays and the bases
 * [x + 1, x + 1 + d) go, all inside the interval.  A pair with x + d >= end is no deletion: valid 0, values 0, enc -1.  The result of
 * (x, d) is what fasim_score_variants defines for pos = x, REF = record[x, x + d + 1), ALT = record[x], with the one difference that
 * the window is the shared context: with c0 = x - lo, REF has the target C, the mark [c0, c0 + d + 1) and the edges (lo > 0, hi <
 * record length); ALT has the target C without the letters [c0 + 1, c0 + 1 + d), the mark [c0, c0 + 1) and the same edges; the clip
 * bit sits on the first and last column of the problem's own window.  Scoring, classes, the reduction over encodings and
 * 2 * value + bit are section 19's, so a value is never below fasim_score_variants' for the same deletion and flank.
 * value[a][c], enc[a][c]: allele a (0 REF, 1 ALT), strand class c (enc -1: value 0); clipped[a]: bit 0 of the allele's largest
 * 2 * value + bit; clean: all d + 1 bytes of REF are upper-case ACGT (the others are scored through the encode table all the same). */
#define FASIM_MAX_DELETION_LENGTHS 16
typedef struct fasim_del_score {
	int32_t value[2][FASIM_TRACK_CLASSES];
	int8_t enc[2][FASIM_TRACK_CLASSES];
	uint8_t clipped[2]; uint8_t valid, clean;
	uint8_t reserved[4];
} fasim_del_score;
/* deletions: the valid (position, length) pairs; prefix_problems, prefix_cols: as fasim_mutagenesis_stats; own_problems: the
 * own-letter continuations, one per (column at which a deletion ends, encoding) and launch; alt_problems: one per (deletion,
 * encoding); cont_cols: the columns both kinds ran until their dead column; cont_cols_bound: what that would be with no early stop;
 * prefix_s, cont_s: HIP-event seconds of k_mut_prefix_pm and k_mut_jump. */
typedef struct fasim_deletion_stats {
	int64_t intervals, positions, deletions, launches, prefix_problems, prefix_cols, own_problems, alt_problems, cont_cols, cont_cols_bound;
	double prefix_s, cont_s, total_s;
} fasim_deletion_stats;
/* Scores every (position, length) of nint intervals for nq >= 1 queries: out[(q * npos + k) * nlen + l], positions as in
 * fasim_score_mutagenesis, lengths in the order given.  valid and clean do not depend on the query.  The result of a pair depends on
 * the record, the interval, the flank, the length, the query and the parameters only.  Refused before any GPU work, the engine stays
 * usable: the refusals of fasim_score_mutagenesis, and nlen outside [1, FASIM_MAX_DELETION_LENGTHS], a length outside
 * [1, FASIM_MAX_ALLELE - 1] or lengths that do not ascend strictly (FASIM_E_ARG); a call in which one position alone does not fit a
 * launch (FASIM_E_UNSUPPORTED): with L the longest interval and s = 4 bytes per query row (rounded up to whole workgroup rows),
 * nenc * min(1 + longest length, L) * s must not exceed 256 MB, e.g. H19 under 48 encodings takes lengths up to 495. */
int fasim_score_deletions(fasim_engine* e, const char* const* rnas, const int32_t* rna_lens, int32_t nq,
                          const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec,
                          const fasim_interval* intervals, int64_t nint, int32_t flank, const int32_t* lengths, int32_t nlen,
                          const fasim_params* p, fasim_del_score* out /* [nq * npos * nlen] */, fasim_deletion_stats* stats /* may be NULL */);
/* The table `fasim --mutagenesis --deletions` writes for one query: `# fasim deletions lncRNA=<rna_name> flank=<F> lengths=<d,d,...>`,
 * the column names of fasim_variants_tsv, then one line per clean deletion, intervals in the order given, positions ascending, lengths
 * in their order: line = regions[k].line, chrom, pos (1-based, of the anchor), id = regions[k].name, ref (d + 1 letters), alt (the
 * anchor), per class <Class>_ref <Class>_alt, max_ref max_alt delta rule_ref rule_alt clipped as fasim_variants_tsv prints them;
 * clipped is the bit of the larger of the two alleles' words 2 * max value + clipped.  scores: the pairs of interval k are
 * scores[offsets[k] * nlen .. offsets[k + 1] * nlen) (an interval that was not scored has none); seqs[k]: the end - start letters of
 * interval k (not read for an interval without scores).  Free with fasim_free. */
int fasim_deletions_tsv(const fasim_region* regions, const int64_t* offsets /* [n + 1] */, int64_t n, const fasim_del_score* scores,
                        const char* const* seqs /* [n] */, const int32_t* lengths, int32_t nlen, int32_t flank, const char* rna_name,
                        char** text, int64_t* text_len);
/* ingest helper: upper-cases a DNA record in place (soft-masked genomes such as UCSC hg38 carry repeats in lower
 * case; the reference does not upper-case and treats such letters as unknown, rules.h:286-312, 82-83). */
void fasim_upper_case(char* seq, int64_t n);

/* deterministic synthetic DNA (splitmix64, 2 bits/base; same stream as tools/synth.py) */
void fasim_synth_dna(char* out, int64_t n, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
