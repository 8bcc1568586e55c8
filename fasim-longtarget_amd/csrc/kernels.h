// Host-callable launchers of the gfx950 kernels (defined in kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include "device_types.h"
#include "doomed.h"

namespace fasim {

enum StripedMode { MODE_PRE = 0, MODE_MAX1 = 1, MODE_ALIGN = 2, MODE_REV = 3 };

constexpr int HAZARD_MAX_CHUNKS = 512;   // column chunks (and checkpoints) per hazard unit in the chunked re-run
struct StripedLaunch {
	const uint8_t* tcodes;      // device: target codes
	const uint8_t* qcodes;      // device: query codes (stage-1 or stage-2 coding), length q_total
	const StripedProb* probs;   // device
	int32_t nprob;
	uint32_t* counter;          // device: work-queue head, zeroed by the launcher
	ScoreLut lut;
	int32_t max_qlen;           // largest q_len in the batch (sizes the LDS stripes)
	uint8_t* colmax;            // MODE_PRE: u8 column maxima, same indexing as tcodes
	uint16_t* colmax_w = nullptr;   // MODE_PRE with word == true: u16 column maxima instead
	int32_t* max_out;           // MODE_PRE / MODE_MAX1: per problem (slot = prob.unit) score, 255 = byte overflow
	AlignEnds* ends;            // MODE_ALIGN: per problem (slot = index in probs)
	// chunked hazard re-run (MODE_PRE, byte mode): see StripedArgs in kernels.hip
	const uint16_t* state = nullptr; int32_t state_rows = 0; const int32_t* chunk_cols = nullptr; const int32_t* chunk_base = nullptr; uint8_t* chunk_rows = nullptr; int32_t row_stride = 0;
	int32_t* chunk_out = nullptr;
	bool spread = false;        // one 256-thread workgroup per CU (LDS request padded past half a CU): every wave gets a SIMD of its own
	// non-NULL: run the HBM-window variant (stripes in global scratch instead of LDS) with this scratch of window_bytes >=
	// striped_window_bytes(...); the LDS-resident kernel is used otherwise
	uint8_t* window = nullptr; size_t window_bytes = 0;
};

// scratch the HBM-window variant of k_striped needs for this launch; 0 where the LDS-resident kernel fits (and force is false).
// Bounded by the problems in flight (at most 2048 slots, 512 MB), not by nprob.
size_t striped_window_bytes(StripedMode mode, bool word, int max_qlen, int nprob, bool force);

// word == false: 8-bit semantics (16 stripes); word == true: 16-bit semantics (8 stripes)
// quirk: reproduce the signed lazy-F exit test of the SSW byte kernels (sswNew.cpp:369,590)
hipError_t launch_striped(StripedMode mode, bool word, bool quirk, const StripedLaunch& a, hipStream_t st);

// target codes of every (segment, encoding) unit: tcodes[(seg*nenc + k)*tstride + c]
hipError_t launch_encode(const uint8_t* dna_dev, const int32_t* seg_start, const int32_t* seg_len, int32_t nseg,
	const int32_t* enc_ids, int32_t nenc, const uint8_t* enc_lut /*[48][256] -> code*/, uint8_t* tcodes,
	int32_t tstride, hipStream_t st);

// hits above threshold, ordered by column, per unit.  hits[] entries = (pos << 8) | score
// unit_ids == nullptr: units 0..nunit-1 ; otherwise nunit entries of unit_ids are processed
hipError_t launch_hits(const uint8_t* colmax, const int32_t* unit_ids, const int32_t* unit_len, const int32_t* stage1, int32_t nunit,
	int32_t tstride, uint32_t* hits, uint32_t hits_cap, uint32_t* hits_total, int32_t* hit_off, int32_t* hit_cnt,
	int32_t* thr_out, hipStream_t st);

// chunked hazard re-run (kernels.hip): chunk plan of every hazard unit, and the merge of the groups' private rows
hipError_t launch_hazard_plan(const int32_t* unit_ids, int32_t nlist, const int32_t* unit_len, const int32_t* unit_first, const uint16_t* colmax16,
	int32_t tstride, int32_t target, int32_t hot_thr, int32_t hot_w, int32_t* chunk_cols, hipStream_t st);
hipError_t launch_hazard_merge(const uint16_t* colmax16, uint8_t* colmax, const int32_t* unit_ids, int32_t nlist, const int32_t* unit_len,
	const int32_t* chunk_cols, const int32_t* chunk_base, const int32_t* src_chunk, const int32_t* zero_from, const uint8_t* chunk_rows, int32_t row_stride, int32_t tstride, hipStream_t st);

hipError_t launch_banded(const uint8_t* tcodes, const uint8_t* qcodes, const BandProb* probs, int32_t nprob,
	uint8_t* scratch, BandOut* out, hipStream_t st);

// ---- scan.hip: fused stage-1 + stage-2 systolic kernel ---------------------------------------------
constexpr int SCAN_SNAP_STEPS = 1024;
// one work item of the checkpoint pass: continue unit `unit` from pipeline step `step0` (0, or a multiple of SCAN_SNAP_STEPS:
// from the snapshot taken there) and leave the DP state after columns dump_cols[first .. first + count)
struct ScanDumpItem { int32_t unit, step0, first, count; };
struct ScanLaunch {
	const uint8_t* tcodes; const int32_t* unit_ids; const int32_t* unit_len; int32_t nwork; int32_t tstride;
	uint32_t* counter; const uint8_t* qcodes; int32_t m; int8_t score[25]; uint16_t* colmax16;
	uint2* boundary;      // [unit][tstride] hand-over rows between query tiles; needed when systolic_tiles(m) > 1
	int32_t coarse;       // 1: coarse Q2 test (FASIM_Q2_COARSE=1, for measurements)
	int32_t* unit_hz;     // [unit], zeroed by the caller: |= 1 when the unit needs the stripe-faithful re-run; may be NULL
	int32_t* unit_first = nullptr;          // [unit], preset to INT_MAX by the caller: first step at which a Q2 taint could arise
	// pipeline snapshots: the main pass leaves its whole wave state every SCAN_SNAP_STEPS steps, so that the checkpoint pass of
	// the chunked hazard re-run can start in the middle of a unit (single-tile queries only)
	uint32_t* snap = nullptr;               // [unit][snap_per_unit][systolic_snap_dwords(m)][64 lanes]; NULL: none taken / none to read
	int32_t snap_per_unit = 0;
	// checkpoint variant (dump_items != NULL): work item = one window of one hazard unit
	const ScanDumpItem* dump_items = nullptr;
	const int32_t* dump_cols = nullptr;     // [chunk]: the column after which the DP state of all rows is wanted (ascending within an item)
	uint16_t* dump_state = nullptr;         // [chunk][2][16 * ceil(m/16)]: H, then the reference's E
	// block maxima for the banded stage 3 (band.hip): [unit][tile][ublk_blocks][64 lanes] x 2 bytes; NULL: not wanted
	uint16_t* ublk = nullptr;
	int32_t ublk_blocks = 0;
	// packed-f16 variant of the main pass (option dp_f16; ignored by the checkpoint variant): exact while every score stays below
	// 1 024.  unit_ovf[unit] (zeroed by the caller) is set to 1 for a unit that left that range: everything the pass wrote for it is
	// void and the caller runs it again with f16 = 0
	int32_t f16 = 0;
	int32_t* unit_ovf = nullptr;
	// row maxima (fasim_scan_tfo_profile; ignored by the checkpoint variant): non-NULL selects the ROWS variant of the main pass,
	// which leaves rowmax16[unit][16 * ceil(m/16)] = 2 * (maximum of the row over the unit's real columns) + taint bit
	uint16_t* rowmax16 = nullptr;
	// Q2 tracking past a unit's overflow cut: 1 = to the end of the unit; 0 = the plain main pass (neither checkpoint nor ROWS variant,
	// ceil(m/16) >= 96) stops it 128 steps after a block of steps whose maximum is >= 251 and clean.  From there on only bit 0 of the
	// column maxima can differ, at columns behind the cut, where k_scan_post does not read it
	int32_t q2_past_cut = 1;
};
constexpr int SCAN_UBLK_STEPS = 64;       // pipeline steps per block of maxima
inline int scan_ublk_blocks(int tstride) { return (tstride + 127 + SCAN_UBLK_STEPS - 1) / SCAN_UBLK_STEPS; }
constexpr int SYSTOLIC_MAX_TILES = 31;
int systolic_vs(int m);
int systolic_tiles(int m);     // query tiles of 128 virtual lanes x <= 24 rows (1 for m <= 3072)
bool systolic_fits(int m);
int systolic_snap_dwords(int m); // dwords per lane of one pipeline snapshot
hipError_t launch_scan(const ScanLaunch& L, hipStream_t st);      // hipErrorInvalidValue: query too long for this kernel
hipError_t launch_scan_post(const uint16_t* colmax16, const int32_t* unit_ids, int32_t nwork, const int32_t* unit_len,
	int32_t tstride, const int32_t* stage1_in, uint32_t* hits, uint32_t hits_cap, uint32_t* hits_total, int32_t* hit_off,
	int32_t* hit_cnt, int32_t* thr_out, int32_t* stage1_out, int32_t* flags, const int32_t* unit_hz, hipStream_t st);
// v_pk_maximum3_f16 on n packed pairs (device pointers): out3 = maximum3(a, b, c), out0 = maximum3(a, b, +0); see dp_f16.h
hipError_t launch_maximum3_f16(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out3, uint32_t* out0, int64_t n, hipStream_t st);
hipError_t launch_max16(const uint16_t* colmax16, const int32_t* unit_ids, int32_t nwork, const int32_t* unit_len,
	int32_t tstride, int32_t* out, hipStream_t st);

// ---- track.hip: per-base potential tracks folded from the column maxima of a batch --------------------
// One slice = TRACK_CHUNK positions of one segment: positions [c * TRACK_CHUNK, min(n, (c + 1) * TRACK_CHUNK)) of segment s are
// slice s * nchunk + c.  A slice holds, per class, the maxima of the record bins its positions touch, first bin first.
constexpr int TRACK_CHUNK = 2040;          // 255 lanes x 8 positions: the reversed rows of a slice then span at most 256 aligned groups of 8
constexpr int TRACK_MAX_LDS_BINS = 1024;   // bins of a slice for bin >= 2 (at most 2039 / 2 + 2)
// the enabled encodings by group g = class + 4 * reversed: k[first[g] .. first[g + 1]) are the indices (0 .. nenc) of group g
struct TrackTable { uint8_t k[48]; uint8_t first[9]; };
inline int track_chunks(int max_len) { return (max_len + TRACK_CHUNK - 1) / TRACK_CHUNK; }
// values per class and slice in the output (a multiple of 8): every bin a slice can touch
__host__ __device__ inline int track_slice_stride(int bin) { const int nb = bin == 1 ? TRACK_CHUNK : (TRACK_CHUNK - 1) / bin + 2; return (nb + 7) & ~7; }
// peak of one slice and class (k_track with PEAKS): the slice's maximum, its smallest position within the SEGMENT, and the smallest
// index k (0 .. nenc) of an enabled encoding of the class whose unit attains it there; value 0: pos = k = -1
struct TrackPeak { int32_t value, pos, k, pad; };
// What the three column folds (k_track, k_sites, k_hist) share: their front half (class_fold.h) reads nothing else
struct ClassFoldLaunch {
	const uint16_t* colmax16;   // [seg * nenc + k][tstride]: 2 * column maximum + taint bit, as k_scan's main pass leaves it
	const int32_t* seg_len;     // [nseg]
	int32_t nseg, nenc, tstride, nchunk;
	TrackTable tab;
	uint8_t* sat;               // [nseg * nenc], zeroed by the caller: 1 = the unit holds a saturated column maximum (16 383)
};
// What every launcher of a column fold asks first.  true: return *rc (hipSuccess: nothing to launch; hipErrorInvalidValue: a row
// stride that is no multiple of 8, or not 1 .. 48 encodings)
inline bool class_fold_done(const ClassFoldLaunch& L, hipError_t* rc)
{
	if (L.nseg <= 0 || L.nchunk <= 0) { *rc = hipSuccess; return true; }
	if ((L.tstride & 7) != 0 || L.nenc < 1 || L.nenc > 48) { *rc = hipErrorInvalidValue; return true; }
	return false;
}
struct TrackLaunch : ClassFoldLaunch {
	const int32_t* phase;       // [nseg]: record position of the segment's first base, modulo bin
	int32_t bin;                // bin == 0: peaks only, no slices
	uint16_t* out;              // [nseg * nchunk][4][track_slice_stride(bin)]
	TrackPeak* peaks = nullptr; // [nseg * nchunk][4], or NULL: no peaks (the slices of a segment's unused chunks are not written)
};
hipError_t launch_track(const TrackLaunch& L, hipStream_t st);

// ---- sites.hip: runs of positions whose potential reaches a fixed value, from the column maxima of a batch ------------------
// One run of one slice (k_track's slices) and class: positions [start, end) of the SEGMENT, all of potential >= min_value; its largest
// value, the smallest position that attains it, and the smallest index k (0 .. nenc) of an enabled encoding of the class whose unit
// attains it there.
struct alignas(16) SiteRun { int32_t start, end, value_k /* value | k << 16 */, pos; };
struct SitesLaunch : ClassFoldLaunch {
	int32_t min_value;          // 1 <= min_value <= 16 383
	uint32_t* counts;           // [nseg * nchunk][4], zeroed by the caller: runs per slice and class (the counting launch writes it)
	const uint32_t* offsets;    // [nseg * nchunk][4]: exclusive prefix sum of the counts (the emitting launch reads it)
	SiteRun* runs;              // [sum of the counts], in (slice, class, position) order (the emitting launch writes it)
};
hipError_t launch_sites(const SitesLaunch& L, bool emit, hipStream_t st);

// ---- hist.hip: histogram of the potential over the positions of a batch -------------------------------
constexpr int HIST_BINS = 16384;           // values 0 .. 16 383 (the saturated column maximum)
constexpr int HIST_LDS_BINS = 1024;        // values below this are counted in the workgroup's LDS histogram first, the others straight in HBM
// A position of a segment that a neighbouring segment of the record covers too (the head zone [0, zone[2 s]) and the tail zone
// [zone[2 s + 1], n) of segment s) is not counted: its four values go to zones[s][head 0 / tail 1][class][zstride], slot = the
// offset within the zone, and the host counts the maximum of the two sides once.
struct HistLaunch : ClassFoldLaunch {
	const int32_t* zone;        // [nseg][2]: end of the head zone (0: none), begin of the tail zone (seg_len: none); head <= tail
	int32_t zstride;            // >= the longest zone of the batch
	uint32_t* hist;             // [4][HIST_BINS], zeroed by the caller: the batch's counts per class and value
	uint16_t* zones;            // [nseg][2][4][zstride] (zstride == 0: no zones, may be NULL)
};
static_assert(std::is_trivially_copyable<TrackLaunch>::value && std::is_trivially_copyable<SitesLaunch>::value && std::is_trivially_copyable<HistLaunch>::value, "kernel arguments");
hipError_t launch_hist(const HistLaunch& L, hipStream_t st);
// k_hist_pairs: k_hist's counts and, beside them, pairs[class][min(P[x - 1], P[x])] for every pair of
// neighbouring positions that lie outside the zones and in one slice.  Two LDS histograms of HIST_PAIR_LDS_BINS values each.
// The zones grow by one position on their interior side: the head zone of segment s is [0, zone[2 s]] (slot = the position), its
// tail zone [zone[2 s + 1] - 1, n) (slot = the position - (zone[2 s + 1] - 1)), so zstride > the longest zone; both are written
// whether the segment has such a neighbour or not.  border[s][chunk][first 0 / last 1][class] is the potential at the first and
// last position of every slice that has positions: the host counts the pairs across the slice borders and the zone borders.
constexpr int HIST_PAIR_LDS_BINS = 512;
struct HistPairsLaunch : HistLaunch {
	uint32_t* pairs;            // [4][HIST_BINS], zeroed by the caller
	uint16_t* border;           // [nseg][nchunk][2][4]
};
static_assert(std::is_trivially_copyable<HistPairsLaunch>::value, "kernel arguments");
hipError_t launch_hist_pairs(const HistPairsLaunch& L, hipStream_t st);

// ---- scan_short.hip: column maxima of a short oligo ----------------------------------------------------
constexpr int SCAN_SHORT_MAX = 112;        // longest oligo k_scan_short takes (FASIM_MAX_OLIGO)
// W(m): the alignments that decide a column maximum start at most this many columns before it
int scan_short_warmup(int m);
struct ScanShortLaunch {
	const uint8_t* tcodes; const int32_t* unit_len; int32_t nunit, tstride;      // as ScanLaunch: units 0 .. nunit - 1, tstride a multiple of 16
	const uint8_t* qcodes; int32_t m;          // the oligo's codes of the stage-2 alphabet, 1 <= m <= SCAN_SHORT_MAX
	int32_t stretch, npairs, warm;             // columns per stretch, stretch pairs per unit, warm-up columns: from scan_short_shape
	uint16_t* colmax16;                        // [unit][tstride] = 2 * column maximum (taint bit 0) for columns < unit_len; the others are 0 or not written
	// non-NULL selects k_scan_short_rows: [unit][pair][16 * ceil(m / 16)] = 2 * row maximum over the real columns of
	// the pair's two stretches; the parts of pairs with 2 * pair * stretch >= unit_len are not written
	uint16_t* rowpart16;
};
// stretch length (a multiple of 16, >= warm), pairs per unit (2 * npairs * stretch >= tstride) and warm-up (W(m) rounded up to 16)
void scan_short_shape(int m, int tstride, int nunit, int* stretch, int* npairs, int* warm);
hipError_t launch_scan_short(const ScanShortLaunch& L, hipStream_t st);      // hipErrorInvalidValue: a shape the kernel does not take

// ---- site_align.hip: the textbook local alignment behind a site's peak -----------------------------------
// One problem: a unit (its target codes at tcodes + tbase, n columns), the column jp of the site's peak and the peak's value.
struct SiteAlignProb { int64_t tbase; int32_t n, jp, value, pad; };
// What k_site_ends leaves for a problem: the end cell (i1, j1) and the start cell (i0, j0) of the hit.  i1 == -1: the unit does
// not hold `value` in column jp; i0 == -1 (with i1 >= 0): the anchored reverse pass did not reach `value`.
struct alignas(16) SiteAlignEnds { int32_t i1, j1, i0, j0; };
// The 16-bit row state clamps at -30 000 ("no alignment") and 32 767: +5 per column cannot climb from the clamp back to a value >= 1
// and a local score stays below the upper clamp only while a unit has at most 6 000 columns (-c); longer units are left unaligned
constexpr int SITE_ALIGN_MAX_COLS = 6000;
constexpr int SITE_ALIGN_LDS_ROWS = 8192;       // query rows whose DP state (7 bytes per row) k_site_ends keeps in LDS
constexpr int64_t SITE_ALIGN_MAX_CELLS = (int64_t)1 << 26;      // largest rectangle k_site_path takes (one direction byte per cell; 4 x 4 096 x 4 096), at most SITE_ALIGN_LDS_ROWS rows
struct SiteEndsLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; int32_t m;      // query codes of the stage-2 alphabet, m real rows (no pad rows)
	int32_t npad;                 // pad rows of the scan (16 * ceil(m/16) - m): their echoes reach npad columns past the real cell
	const SiteAlignProb* probs; int32_t nprob;
	int16_t* rows;                // [nprob][3][m]: DP state of the queries that do not fit the LDS (m > SITE_ALIGN_LDS_ROWS), else NULL
	SiteAlignEnds* ends;          // [nprob]
};
// One path: the rectangle [i0, i1] x [j0, j1] of problem `prob`; direction bytes at dirs + dir_off (rows * cols of them), the
// CIGAR (BAM encoding, LAST operation first) at cigar + cig_off, at most cig_cap words
struct SitePathItem { int64_t dir_off; int32_t prob, i0, i1, j0, j1, cig_off, cig_cap, pad; };
struct SitePathLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; const SiteAlignProb* probs;
	const SitePathItem* items; int32_t nitem;
	int32_t max_rows;             // the tallest rectangle of the launch, at most SITE_ALIGN_LDS_ROWS
	uint8_t* dirs; uint32_t* cigar;
	int32_t* cigar_len;           // [nitem]: words written, -1: the anchored pass did not give `value` or the path left the rectangle
};
hipError_t launch_site_ends(const SiteEndsLaunch& L, hipStream_t st);
hipError_t launch_site_path(const SitePathLaunch& L, hipStream_t st);

// ---- site_short.hip: k_site_ends for an oligo, one problem per lane over a window of the unit ------------
// k_site_ends_short<ROWS>, ROWS = 16 * ceil(m / 16) in {16, ..., 112}: the same problems in, the same SiteAlignEnds out as
// k_site_ends, for queries of 1 <= m <= SCAN_SHORT_MAX nt (L.rows is not used; L.npad must be 16 * ceil(m / 16) - m)
int site_short_warm(int m);             // columns before (jp & ~15) at which pass (i) starts from zeros: W(m) + 16 rounded up to 16
hipError_t launch_site_ends_short(const SiteEndsLaunch& L, hipStream_t st);      // hipErrorInvalidValue: a query the kernel does not take

// ---- variant.hip: the best local alignment through a variant, per allele window and encoding ------------
constexpr int TOUCH_MAX_COLS = 5120;            // columns of an allele window: FASIM_MAX_ALLELE + 2 * FASIM_MAX_FLANK (the 16-bit row state holds 2 * 5 * 5 120 + 1)
constexpr int TOUCH_LDS_ROWS = 8192;            // query rows whose DP state (7 bytes per row) k_touch keeps in LDS
// One problem: window `win` (a HapWindow, below) under encoding `enc`; its n target codes at tcodes + tbase, the allele's columns [v0, v1) (mirrored for an
// odd encoding, as the codes are), edge bit 0 / 1: the unit's first / last column is an end that the flank cut
struct TouchProb { int64_t tbase; int32_t n, v0, v1, edge, win, enc; };
struct TouchLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; int32_t m;      // query codes of the stage-2 alphabet, m real rows (no pad rows)
	const TouchProb* probs; int32_t nprob;
	uint16_t* rows;               // [nprob][3][touch_state_rows(m)]: DP state of the queries that do not fit the LDS (m > TOUCH_LDS_ROWS), else NULL
	uint32_t* out;                // [nprob]: 2 * value + clip bit
};
// problems of a launch in (variant, allele, k) order, k = index into enc[0 .. nenc); out[variant][9]: per (allele, class) word
// (2 * value + b) << 8 | smallest encoding that attains the value (0xff: value 0), then the variant's clipped flag
struct TouchReduceLaunch { const uint32_t* touch; int32_t nvar, nenc; uint8_t enc[48]; uint32_t* out; };
int touch_threads(int m);        // threads of k_touch's workgroup: 64, 128 or 256
int touch_state_rows(int m);     // 16-bit words per array of a problem's row state: m rounded up to whole rows-per-thread x threads
hipError_t launch_touch(const TouchLaunch& L, hipStream_t st);
hipError_t launch_touch_reduce(const TouchReduceLaunch& L, hipStream_t st);
// k_touch_path: the path behind a value.  One item = problem `prob` of the launch that k_hap_encode served,
// with the plain value its unit attains; its direction bytes at dirs + dir_off ([n][touch_state_rows(m)]), its CIGAR words (last
// operation first, (len << 4) | op) at cigar + cig_off, at most cig_cap of them
constexpr int64_t TOUCH_PATH_MAX_CELLS = (int64_t)1 << 26;      // m * n of a problem that is traced
struct TouchPathItem { int64_t dir_off; int32_t prob, value, cig_off, cig_cap; };
struct TouchPathOut { int32_t i1, j1, i0, j0, cigar_len, pad[3]; };      // cigar_len -1: no path (cells as far as they were found, else -1)
struct TouchPathLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; int32_t m;
	const TouchProb* probs; const TouchPathItem* items; int32_t nitem;
	uint16_t* rows;               // [nitem][3][touch_state_rows(m)] where m > TOUCH_LDS_ROWS, else NULL
	uint8_t* dirs; uint32_t* cigar; TouchPathOut* out;      // out[nitem]
};
hipError_t launch_touch_path(const TouchPathLaunch& L, hipStream_t st);

// ---- haplotype.hip: allele windows assembled from pieces, in the letters of the record or of a haplotype (DESIGN.md sections 19, 25) --
// A window is npiece pieces in window order, pieces[piece0 .. piece0 + npiece): a stretch of the record (alt 0: letters from dna +
// src) or of an uploaded ALT string (alt 1: from alts + src); ends[piece0 + k] is the number of window letters up to and including
// piece k, so the last one is the window's length.  A problem is a TouchProb whose `win` names a HapWindow: k_hap_encode fills
// tcodes[tbase + c], c in [0, n), with the code of window letter c (n - 1 - c for an odd encoding) under the problem's encoding.
constexpr int HAP_LDS_PIECES = 64;              // piece ends of a window that k_hap_encode searches in LDS; the rest it searches in HBM
struct HapPiece { int64_t src; int32_t alt, pad; };
struct HapWindow { int64_t piece0; int32_t npiece, pad; };
struct HapEncodeLaunch {
	const uint8_t* dna; const uint8_t* alts; const HapWindow* wins; const HapPiece* pieces; const int32_t* ends;
	const TouchProb* probs; int32_t nprob; const uint8_t* enc_lut /*[48][256] -> code*/; uint8_t* tcodes;
};
hipError_t launch_hap_encode(const HapEncodeLaunch& L, hipStream_t st);

// ---- mutagenesis.hip: every substitution at every position of an interval from one shared pass -------------
// A unit is one context (interval and flanks) under one encoding with a range of its columns: a TouchProb whose n codes k_hap_encode
// wrote, whose [v0, v1) are the columns of the range's positions (mirrored for an odd encoding, as the codes are) and whose edge bits
// are section 19's.  first[u] counts the columns of the units before u: column v0 + s of unit u has snapshot first[u] + s
// ([2][touch_state_rows(m)] 16-bit words: H of the column before it, then E, in ColState's order) and, for letter b of ACGT, problem
// 4 * (first[u] + s) + b.  k_mut_prefix (one workgroup per unit) writes the snapshots, k_mut_touch (one per problem) out[problem] =
// 2 * value + clip bit and cols[problem] = the columns it ran.
struct MutLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; int32_t m;
	const TouchProb* units; const int32_t* first /*[nunit + 1]*/; int32_t nunit, ncol /* = first[nunit] */;
	const uint8_t* enc_lut /*[48][256] -> code*/;
	uint16_t* rows;               // [max(nunit, problems)][3][touch_state_rows(m)] where m > TOUCH_LDS_ROWS, else NULL
	uint16_t* snap; uint32_t* out; uint32_t* cols;
};
// A group is the nenc units [unit0, unit0 + nenc) of one context and one range of npos positions, in the order of enc[]; the group's
// position j is column v0 + j of an even and v1 - 1 - j of an odd encoding.  out[(pos0 + j)][20]: per (letter, class) k_touch_reduce's
// word, then per letter the columns its problems ran.
struct MutGroup { int32_t unit0, pos0, npos, pad; };
struct MutReduceLaunch {
	const uint32_t* touch; const uint32_t* cols; const int32_t* first; const MutGroup* groups; int32_t ngroup, npos, nenc; uint8_t enc[48];
	uint32_t* out;
};
constexpr int MUT_WORDS = 20;
hipError_t launch_mut_prefix(const MutLaunch& L, hipStream_t st);
hipError_t launch_mut_touch(const MutLaunch& L, hipStream_t st);      // 4 * ncol problems
hipError_t launch_mut_reduce(const MutReduceLaunch& L, hipStream_t st);
// Every deletion of an interval from the same shared pass.  A group is again one context and one range of npos
// positions under the nenc encodings, but its units' [v0, v1) are the columns of `next` >= npos positions: the range's own and, for
// the deletions that reach beyond it, up to the longest length more, never past the interval's end.  The group's position j (j < next)
// is column v0 + j of an even and v1 - 1 - j of an odd encoding; (j, lengths[l]) with j < npos is a deletion iff j + lengths[l] < next.
// k_mut_prefix_pm writes the snapshots as k_mut_prefix does and pm[first[u] + s], the maximum of the plain H over the real rows of
// column v0 + s as 2 * value + clip bit, for s < v1 - v0 - 1.  A jump problem (s, k, r) loads the snapshot before column s, runs column
// k in plain mode and then the columns from r on, which only continue.  Problems of a launch: [0, ncol) the own-letter problem
// (c, c, c + 1) of every snapshot column c -- run only where it is the last mark column of a deletion of the group: the position
// where one ends (even) or where one is anchored (odd) -- then nalt = npos * nenc *
// nlen ALT problems, ((pos0 * nenc + k * npos + j) * nlen + l) for deletion (j, l) of the group under its k-th encoding.
// k_mut_jump: out[problem] = 2 * value + clip bit, cols[problem] = the columns it ran (both 0 for a problem that is not run).
// k_mut_del_reduce: out[(pos0 + j) * nlen + l][DEL_WORDS]: per (allele, class) k_touch_reduce's word, then the columns run by the
// deletion's ALT problems and by the own-letter problems it is the first to use (the smallest l of the group with that last mark
// column), then whether it is a deletion.
struct DelGroup { int32_t unit0, pos0, npos, next; };
struct DelLaunch {
	const uint8_t* tcodes; const uint8_t* qcodes; int32_t m;
	const TouchProb* units; const int32_t* first /*[nunit + 1]*/; int32_t nunit, ncol /* = first[nunit] */;
	uint16_t* rows;               // [max(nunit, ncol + nalt)][3][touch_state_rows(m)] where m > TOUCH_LDS_ROWS, else NULL
	uint16_t* snap; uint32_t* pm /*[ncol]*/; uint32_t* out /*[ncol + nalt]*/; uint32_t* cols /*[ncol + nalt]*/;
	const DelGroup* groups; int32_t ngroup, npos, nenc, nlen, nalt;
	int16_t lengths[16]; uint8_t enc[48];
	uint32_t* words;              // [npos * nlen][DEL_WORDS]
};
constexpr int DEL_WORDS = 10;
hipError_t launch_mut_prefix_pm(const DelLaunch& L, hipStream_t st);
hipError_t launch_mut_jump(const DelLaunch& L, hipStream_t st);      // ncol + nalt problems
hipError_t launch_mut_del_reduce(const DelLaunch& L, hipStream_t st);

// ---- rowfold.hip: per-base profile of the lncRNA folded from the row maxima of a batch -------------------------
// Group g = segments [gfirst[g], gfirst[g + 1]) of the batch (the run of segments of one record, or the whole batch); the result is
// out[g][4 classes][rows_total] = maximum over the group's units of the class, taint bit dropped.
struct RowFoldLaunch {
	const uint16_t* rowmax16;   // [seg * nenc + k][rows_total], as the ROWS variant of k_scan leaves it
	const int32_t* gfirst;      // [ngroups + 1]
	int32_t ngroups, nenc, rows_total;      // rows_total: a multiple of 16
	TrackTable tab;
	uint16_t* out;              // [ngroups][4][rows_total]
	uint8_t* sat;               // [nseg * nenc], zeroed by the caller: 1 = the unit holds a saturated row maximum (16 383)
};
hipError_t launch_rowfold(const RowFoldLaunch& L, hipStream_t st);
// k_rowfold_parts: the same result from the parts k_scan_short_rows leaves, out[g][4 classes][rows] = maximum over the group's units of
// the class and over their written parts, taint bit dropped
struct RowPartFoldLaunch {
	const uint16_t* rowpart16;  // [(seg * nenc + k) * npairs + pair][rows]
	const int32_t* unit_len;    // [nseg * nenc]
	const int32_t* gfirst;      // [ngroups + 1]
	int32_t ngroups, nenc, rows, npairs, stretch;      // rows: a multiple of 16, at most 112; npairs and stretch: the scan's
	TrackTable tab;
	uint16_t* out;              // [ngroups][4][rows]
};
hipError_t launch_rowfold_parts(const RowPartFoldLaunch& L, hipStream_t st);

// ---- align.hip: stage 3 ---------------------------------------------------------------------------
struct FwdLaunch {
	const uint8_t* stream; const FwdProb* probs; const int32_t* task_first; int32_t ntask; uint32_t* counter;
	const uint8_t* qcodes; int32_t m; FwdOut* out;
	uint4* boundary;      // [stream position] hand-over between query tiles; needed when systolic_tiles(m) > 1
	int32_t word;         // 1: the reference's 16-bit pass (no overflow rule, no Q2): plain variant without taint tracking
	// reverse pass (word == 1, lane_ub != NULL): reversed query against reversed windows; leaves per window (slot ub_slot[k], -1:
	// none) and zone 0..3 the per-lane maxima [slot][4][128 * tiles] and writes no FwdOut
	uint16_t* lane_ub = nullptr; const int32_t* ub_slot = nullptr;
	int32_t f16 = 0;      // reverse pass only: 1 = the packed-f16 variant (option dp_f16), same lane maxima
};
// zones: NULL, or (reverse pass) per window the lengths of the candidate's next three tries (bytes 0..2; 0 = none): the stream then
// holds the REVERSED window with the zone of every column in bits 5-6
hipError_t launch_build_stream(const uint8_t* tcodes, const FwdProb* probs, int32_t nprob, uint8_t* stream, const uint32_t* zones, hipStream_t st);
hipError_t launch_align_fwd(const FwdLaunch& L, hipStream_t st);     // hipErrorInvalidValue: query too long
hipError_t launch_finish(const uint8_t* tcodes, const uint8_t* qcodes, const FwdProb* probs, const FwdOut* fwd, const int32_t* order,
	int32_t nprob, uint8_t* dirs, AlignOutDev* out, uint32_t* cigar_pool, uint32_t pool_cap, uint32_t* pool_count, hipStream_t st);
// The split tier 1 (k_finish_rev, k_finish_compact, k_finish_trace): what the rule of doomed.h needs on the device.  The batch's DNA
// letters with the segment starts and lengths k_encode read them by, the enabled encodings, per segment 1 = only ACGTN (complement()
// drops nothing).  check: 1 = mark the alignments the rule would skip in marks[] and trace them all the same (option finish_skip = 2).
struct FinishSkip {
	const uint8_t* dna; const int32_t* seg_start; const int32_t* seg_len; const int32_t* enc_ids; const uint8_t* seg_clean;
	int32_t nenc, tstride, check;
	DoomedParams dp;
};
hipError_t launch_finish_split(const uint8_t* tcodes, const uint8_t* qcodes, const FwdProb* probs, const FwdOut* fwd, const int32_t* order,
	int32_t nprob, uint8_t* dirs, AlignOutDev* out, uint32_t* cigar_pool, uint32_t pool_cap, uint32_t* pool_count, const FinishSkip& fs,
	uint64_t* masks, int32_t* list, uint32_t* list_count, uint8_t* marks, hipStream_t st);

hipError_t launch_finish_mid(const uint8_t* tcodes, const uint8_t* qcodes, const FwdProb* probs, const FwdOut* fwd, const int32_t* idx_list,
	int32_t nlist, uint8_t* dirs, AlignOutDev* out, uint32_t* cigar_pool, uint32_t pool_cap, uint32_t* pool_count, hipStream_t st,
	const FinishSkip* fs = nullptr /* non-NULL: the rule of doomed.h as an exit behind the reverse pass */, uint8_t* marks = nullptr /* fs->check */);
hipError_t launch_finish_big(const uint8_t* tcodes, const uint8_t* qcodes, const FwdProb* probs, const FwdOut* fwd,
	const int32_t* idx_list, int32_t nlist, uint8_t* scratch, int32_t scratch_cap, AlignOutDev* out, uint32_t* cigar_pool,
	uint32_t pool_cap, uint32_t* pool_count, hipStream_t st);

// ---- band.hip: banded forward pass of stage 3 -------------------------------------------------------------
// one selected try: the band kernel sweeps rows [r0, r0 + 48 G) of window `prob`; its result is the reference's iff the
// score reaches theta_min; nq = length of the try's column stream in groups of 4 columns
struct BandTry { int32_t prob, r0, theta_min, nq; };
constexpr int BAND_SLOT_COLS = 208;       // 16-bit stream words per try (window <= 200 columns + 2 void columns, rounded up to 4)
constexpr int BAND_MAX_ZONES = 32;          // 31 zones of 64 profile lanes hold the longest query
// counters of one selection pass: [class * BAND_MAX_ZONES + zone] tries, then stream columns per class, then (debug) the tries left
// unbanded because a bound reaches 148 / because no band proves the target
constexpr int BAND_COUNT_COLS = 3 * BAND_MAX_ZONES, BAND_COUNT_HOT = BAND_COUNT_COLS + 3, BAND_COUNT_NOBAND = BAND_COUNT_COLS + 4, BAND_COUNTS = 128;
struct BandSelLaunch {
	const FwdProb* probs; const int32_t* target; const int32_t* idx; int32_t n, tstride;
	const uint16_t* ublk; int32_t ublk_blocks; int32_t m; const uint8_t* tcodes;
	// start-based bounds from the reverse pass of the candidate (k_align_fwd's lane maxima over the reversed problem):
	// prev[k] = slot * 4 + zone (zone 0..3) or -1 (then the block maxima of k_scan bound the try); NULL: none
	const uint16_t* prev_ub = nullptr; const int32_t* prev = nullptr;
	BandTry* list[3]; uint16_t* slots[3]; uint32_t list_cap;
	int4* dec;                // [n] decisions (decide -> emit)
	uint32_t* counts;         // [BAND_COUNTS], zeroed and filled by launch_band_decide
	uint32_t* cursors;        // [3 * BAND_MAX_ZONES] first slot of every (class, zone) segment, consumed by launch_band_emit
	FwdOut* out; int32_t class_mask;
	int32_t debug = 0;        // 1: count the tries left unbanded by reason
};
// one workgroup of a band launch: profile lanes [zbase, zbase + lc) staged in LDS, tries list[first .. first + count) shared by
// the `nwg` workgroups of the zone (this one is number `wg`)
struct BandZoneTab { int32_t zbase, first, count, wg, nwg; };
struct BandLaunch { const BandTry* list; const uint16_t* slots; const BandZoneTab* tab; int32_t nwg, cls; const uint8_t* qcodes; int32_t m; FwdOut* out; };
int band_profile_lanes(int m);
int band_zone_stride(int m);          // profile lanes per zone (== band_profile_lanes(m) for queries that need one zone)
int band_classes(int m);              // bit c set: class c (sub-pipelines of 8 << c lanes = 384 << c rows) is available for this query
std::vector<BandZoneTab> band_plan(int m, int cls, const uint32_t* zone_count, const uint32_t* zone_first);
hipError_t launch_band_decide(const BandSelLaunch& L, hipStream_t st);
hipError_t launch_band_emit(const BandSelLaunch& L, hipStream_t st);
hipError_t launch_align_band(const BandLaunch& L, hipStream_t st);

// ---- sim.hip: forward sweep of classic SIM (-F), one wave per unit ---------------------------------------
hipError_t launch_sim_forward(const SimFwdArgs& a, int32_t nunit, hipStream_t st);
hipError_t launch_sim_resweep(const SimResweepArgs& a, int32_t nunit, bool few_units, hipStream_t st);
bool sim_resweep_in_lds(const SimResweepArgs& a, bool few_units);      // the variant that launch takes: k_sim_resweep<true> (lines' states in LDS) or <false>

} // namespace fasim
