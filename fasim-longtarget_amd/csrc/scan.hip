// fasim-longtarget_amd/csrc/scan.hip -- the fused stage-1 + stage-2 "scan" kernel for gfx950.
//
// Textbook Gotoh recurrence over the whole (query x 5 kb segment) matrix of a
// unit, as the systolic pipeline of systolic.h inside ONE wave64 (128 virtual lanes of RP rows each, packed
// 16-bit VALU, ~10 instructions per pair of cells; no MFMA: this is integer DP):
//   * the int16 query profile (5 target codes x rows) is staged once per workgroup in LDS;
//   * the segment's target codes are read 64 columns at a time (one coalesced byte per lane) and fed to
//     virtual lane 0 with v_readlane; per-column maxima leave virtual lane 127 as one u16 per step.
//
// What it replaces: calc_score_once() (stats.h:879-956) and sw_sse2_byte_once() (sswNew.cpp:255-464) for
// every unit in which the reference's layout-dependent behaviour cannot show: the column maxima are the
// textbook ones up to the reference's overflow column (Q1, applied in k_scan_post) unless the signed
// lazy-F exit (Q2, sswNew.cpp:369) can trigger.  Q2 needs an F value >= 132 to cross one of the 15 stripe
// boundaries k*ceil(m/16) of the reference's striped layout.  The rows are laid out so that each of the
// reference's 16 stripes is exactly `vs` virtual lanes: the F entering virtual lane vs*k IS the F crossing
// boundary k.  Zero-score pad rows (Q3) are part of the profile.
//
// Taint tracking.  Every DP value is carried DOUBLED, with bit 0 = "the reference may hold a smaller value here
// because of Q2".  Doubled scores and gap costs are even, so the bit rides through add / saturating subtract for
// free, and max() keeps it exactly when the winning operand carries it (ties go to the tainted operand, which is
// the safe side).  The hazard test sets the bit on the cells whose value the reference's early lazy-F exit would
// have withheld; a unit needs the stripe-faithful re-run (kernels.hip) only if a tainted value ends up as a column
// maximum that matters (above the threshold or at the overflow cut: k_scan_post).  Second-order effects stay on the
// safe side: the reference's values are never larger than the textbook ones, so a chain that is hot there is hot
// here; a tainted H counts as "< 144" in the arming test; and a tainted H or F can only produce tainted results.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include "kernels.h"
#include "systolic.h"

namespace fasim {

// two carried maxima (2 * value + taint each) -> two bytes min(value, 255)
__device__ __forceinline__ uint16_t ublk_pack(v2u acc)
{
	const v2u v = __builtin_elementwise_min(acc >> (v2u){ 1, 1 }, (v2u){ 255, 255 });
	return (uint16_t)(v[0] | (v[1] << 8));
}

constexpr int SCAN_DEAD = -16384;           // score of rows beyond the padded query: can never be chosen

struct ScanArgs {
	const uint8_t* tcodes;       // [unit][tstride]
	const int32_t* unit_ids;     // work list (indices into tcodes/unit_len), nwork entries
	const int32_t* unit_len;
	int32_t nwork;
	int32_t tstride;
	uint32_t* counter;
	const uint8_t* qcodes;       // query codes for this scoring (0..4)
	int32_t m;                   // query length
	int32_t m_pad;               // 16 * ceil(m/16): rows [m, m_pad) score 0 (Q3)
	int32_t seg_len16;           // ceil(m/16): stripe length of the reference's byte kernels
	int8_t score[25];            // score[t*5+q]
	uint16_t* colmax16;          // [unit][tstride] : 2 * column maximum + taint bit (32767 = saturated)
	int32_t* unit_hz;            // [unit] |= 1: the whole unit needs the stripe-faithful re-run (NULL: not tracked)
	int32_t coarse;              // 1: unit-level test only (any F[b] >= 132), no row analysis
	int32_t vs;                  // virtual lanes per reference stripe (multiple of 8): 16*vs virtual lanes in all
	int32_t tile;                // this launch handles virtual lanes [128*tile, 128*tile+128)
	int32_t ntiles;
	uint2* boundary;             // [unit][tstride]: per column {hbot | fbot<<16, cm | fpo<<16} handed from tile to tile
	int32_t* unit_first;         // [unit] atomicMin: first pipeline step at which a Q2 taint could arise (NULL: not tracked)
	uint32_t* snap;              // pipeline snapshots [unit][snap_per_unit][2 * RP + 6][64] (main pass: written; DUMP: read); may be NULL
	int32_t snap_per_unit;
	// DUMP variant only (checkpoints for the chunked hazard re-run): work item w = dump_items[w] continues a unit from a
	// snapshot (or from step 0) and leaves H and the reference's E of every row after columns dump_cols[first .. first + count)
	// in dump_state[chunk][2][rows_total] (values as carried: 2 * value + taint)
	const ScanDumpItem* dump_items;
	const int32_t* dump_cols;
	uint16_t* dump_state;
	int32_t rows_total;          // 16 * ceil(m/16)
	// block maxima for the banded stage 3 (band.hip): per unit, query tile and block of SCAN_UBLK_STEPS pipeline steps two bytes per
	// lane = the maximum H (capped at 255: anything from 148 on only means "not banded") over the rows of the lane's two virtual
	// lanes and the steps of the block; virtual lane v of the tile sees column c at step c + v.  [unit][tile][block][64 lanes]; NULL: not wanted
	uint16_t* ublk;
	int32_t ublk_blocks;         // blocks per (unit, tile) in the buffer
	int32_t* unit_ovf;           // F16 variant: [unit] = 1 when some H left the exact range (>= 2048 as carried): the unit's outputs are void
	// ROWS variant only (fasim_scan_tfo_profile): [unit][rows_total] row maxima over the unit's real columns, as carried
	// (2 * value + taint), folded per class by k_rowfold (rowfold.hip)
	uint16_t* rowmax16;
	// 0: Q2 tracking stops once a block maximum proves the unit's overflow cut (below); 1: tracking runs to the end of the unit.
	// Only the plain main-pass builds (neither DUMP nor ROWS, RP >= 12) with long stripes (ceil(m/16) >= 96) look at it.
	int32_t q2_past_cut;
};

// score of target code t against the r-th row of global virtual lane v (doubled: bit 0 is the taint bit)
__device__ __forceinline__ int scan_cell_score(const ScanArgs& a, int t, int v, int r)
{
	int row0, rows_v;
	lane_rows(v, a.seg_len16, a.vs, &row0, &rows_v);
	if (r >= rows_v) return SCAN_DEAD;
	const int row = row0 + r;
	if (row < a.m) return 2 * a.score[t * 5 + a.qcodes[row]];
	return 0;                                 // rows [m, 16*segLen) are the reference's zero-score pad rows (Q3)
}

// One 256-thread workgroup shares the per-code int16 profile (35 KB); the two halves of a lane fetch their own code's rows and a
// v_perm_b32 per row merges them.  (A variant with the profile stored per PAIR of codes -- no perm, 109 KB of LDS, 1024-thread
// workgroups -- was 5 % faster alone and 1-4 % slower with ten batches in flight; it was removed in round 3.)
//
// F16 (main pass only): the same values, "2 x value + taint bit", carried as f16 integers, with the row pair of dp_f16.h.  An odd
// value is tainted: doubled scores and gap costs are even, so parity rides through add and subtract as the bit does, and
// 2h + 1 > 2h, so a maximum prefers the tainted operand.  All of it is exact while values stay <= 2047 (scores <= 1023).
// Rounding above 2048 is monotone and every H is seen by the block maxima, so a unit that ever held a value outside the exact
// range shows a block maximum >= 2048: it is flagged in unit_ovf, its outputs are void, and the host runs it again on the
// integer kernel.  Everything that leaves the pipe (column maxima, block maxima, snapshots) leaves as the integers of the
// integer kernel; the hand-over between query tiles carries the f16 bits.
//
// ROWS (main pass only, fasim_scan_tfo_profile): the wave also keeps the running maximum of every row it
// owns, RP more packed registers, and stores them to rowmax16[unit][row] at the end of the unit.  Rows are private to a virtual
// lane, so nothing is handed over between lanes or tiles.  Only real columns count: in the last 127 steps of a unit a half may
// be working on a drain column >= n (fed with code N), whose diagonal H[i-1][n-1] - 4 can exceed everything row i really holds,
// so those steps run a second instantiation of the step body that masks such a half out of the accumulation.  The fill steps
// need nothing (state and values are zero there).  The large RP no longer fit 128 VGPRs: they are built for 3 waves per SIMD.
//
// Q2 past the cut (plain main pass, q2_past_cut = 0).  k_scan_post reads the taint bit of a column maximum
// only at columns <= cut, the first column whose (textbook) maximum reaches 251.  A block maximum that is >= 251 and clean is such
// a value, and the reference's own: it sits in a column c' <= the block's last step, so cut <= c'.  Virtual lane 127 finishes
// column c' at step c' + 127; from 128 steps after the block's last step on every lane works on a column > c', whose taints
// nothing reads, and the steps leave the hazard branch out (fpo = 0, as when its superset test is false).  The decision is a
// scalar one, taken where the block closes; a step pays a scalar compare for it.
constexpr int scan_rows_waves(int RP, bool F16) { return RP >= (F16 ? 18 : 20) ? 3 : 4; }
template <int RP, bool DUMP = false, bool F16 = false, bool ROWS = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DUMP ? 1 : (ROWS ? scan_rows_waves(RP, F16) : 4), DUMP ? 2 : 4))) k_scan(ScanArgs a)
{
	static_assert(!(F16 && DUMP), "the checkpoint pass is an integer pass");
	static_assert(!(ROWS && DUMP), "the checkpoint pass keeps no row maxima");
	extern __shared__ __align__(16) uint8_t prof[];
	const int lane = threadIdx.x & 63;

	// ---- stage the int16 profile: this launch stages the rows of its tile only -------------------------
	stage_profile<F16, SCAN_DEAD>(prof, 5, a.tile, [&](int t, int v, int r) { return scan_cell_score(a, t, v, r); });
	__syncthreads();

	// ---- per-lane constants: Q2 needs F[b] >= 132 (doubled: > 263) ---------------------------------------
	const StripeLane ln(128 * a.tile + 2 * lane, a.seg_len16, a.vs, RP, F16 ? f16c(263u) : 263u);
	const uint32_t act = ln.act;
	const v2u actm = ln.actm, startm = ln.startm;
	// the refined test needs F to die inside one stripe (F <= 234 decays by 4 per row)
	const bool lvl2 = a.seg_len16 >= 96 && !a.coarse;
	// the builds that may stop the tracking behind a proven cut, and whether this launch asks for it
	// (long stripes take 12 rows per lane or more: ceil(m/16) >= 96 with 8 virtual lanes per stripe up to 192)
	constexpr bool PAST_CUT = !DUMP && !ROWS && RP >= 12;
	const bool cut_stops = PAST_CUT && lvl2 && a.q2_past_cut == 0;
	const uint8_t* pl = prof + lane * PROF_LANE_STRIDE;

	for (;;) {
		int w = 0;
		if (lane == 0) w = (int)atomicAdd(a.counter, 1u);
		w = __builtin_amdgcn_readfirstlane(w);
		if (w >= a.nwork) break;
		ScanDumpItem item = { 0, 0, 0, 0 };
		if constexpr (DUMP) item = a.dump_items[w];
		const int unit = DUMP ? item.unit : a.unit_ids[w];
		const int n = a.unit_len[unit];
		const uint8_t* tc_unit = a.tcodes + (int64_t)unit * a.tstride;
		uint16_t* out = a.colmax16 + (int64_t)unit * a.tstride;
		uint2* bnd = a.boundary + (int64_t)unit * a.tstride;
		const bool first_tile = a.tile == 0, last_tile = a.tile == a.ntiles - 1;
		uint2 bchunk = make_uint2(0u, 0u);

		// H and E are kept as plain 32-bit registers (two packed u16 halves each) and only viewed as vectors inside the
		// arithmetic: vector-typed loop-carried values get split into halves and re-packed by the compiler
		int H[RP], E[RP];
#pragma unroll
		for (int r = 0; r < RP; r++) { H[r] = 0; E[r] = 0; }
		int tc = 0x00040004;          // target codes of my two halves (N = neutral while the pipeline fills)
		int hbot = 0, fbot = 0, cm = 0, recv_h_last = 0, fpo = 0;
		v2u hzacc = (v2u){ 0, 0 };      // != 0: the unit goes to the stripe-faithful kernel (coarse test of short queries)
		int chunk = CODE_N;
		int first_enter = 0x7fffffff;          // first step of this unit in which the hazard branch ran (wave-uniform)
		v2u ubacc = (v2u){ 0, 0 };             // running maximum of the current block of steps (banded stage 3)
		bool ovf = false;                      // F16: some block maximum of this unit reached 2048, the end of the exact range (wave-uniform)
		// PAST_CUT: the row analysis runs in the steps < q2_until: none with short stripes, all until a clean block maximum has proven the cut (wave-uniform)
		int q2_until = lvl2 ? 0x7fffffff : (int)0x80000000;
		// DUMP only: the reference's OWN E.  Its lazy-F loop corrects H but not E (sswNew.cpp:355: "don't update E"), so E follows
		// the H of the main pass, which only knows the F chain restarted at the top of each stripe (Fm).  The H values are the
		// same either way (a gap pair in the order down-right scores what right-down scores), the E array is not, and a
		// checkpoint has to be the reference's exact state.
		int Es[RP]; int fmbot = 0;
#pragma unroll
		for (int r = 0; r < RP; r++) Es[r] = 0;
		// ROWS only: running maximum of each of my row pairs over the real columns (F16: the bit patterns, which order like the values)
		int RM[ROWS ? RP : 1];
#pragma unroll
		for (int r = 0; r < (ROWS ? RP : 1); r++) RM[r] = 0;
		// checkpoint columns are ascending and a half's column moves up by one per step: each half only watches its NEXT one
		int dlast = -1, dnext[2] = { 0x7fffffff, 0x7fffffff }, dnx[2] = { 0, 0 };
		int drow0[2] = { 0, 0 }, drows[2] = { 0, 0 };
		const int32_t* dc = nullptr;
		constexpr int SNAP_DW = 2 * RP + 6;
		if constexpr (DUMP) {
			dc = a.dump_cols + item.first;
			if (item.count > 0) { dlast = dc[item.count - 1]; dnext[0] = dnext[1] = dc[0]; }
			for (int h = 0; h < 2; h++) lane_rows(128 * a.tile + 2 * lane + h, a.seg_len16, a.vs, &drow0[h], &drows[h]);
			if (item.step0 > 0) {
				// continue from the snapshot the main pass took at the top of step step0.  The reference's E starts as the textbook
				// E and is exact 64 columns later (a surplus decays by the gap extension, 4 a column, from at most 250; the
				// restarted F chain follows within the column): the host only asks for columns >= step0 + 64 here.
				const uint32_t* sp = a.snap + ((size_t)unit * a.snap_per_unit + (item.step0 / SCAN_SNAP_STEPS - 1)) * (SNAP_DW * 64) + lane;
#pragma unroll
				for (int r = 0; r < RP; r++) { H[r] = (int)sp[(2 * r) * 64]; E[r] = (int)sp[(2 * r + 1) * 64]; Es[r] = E[r]; }
				tc = (int)sp[(2 * RP) * 64]; hbot = (int)sp[(2 * RP + 1) * 64]; fbot = (int)sp[(2 * RP + 2) * 64]; cm = (int)sp[(2 * RP + 3) * 64];
				recv_h_last = (int)sp[(2 * RP + 4) * 64]; fpo = (int)sp[(2 * RP + 5) * 64];
			}
		}
		// (the DUMP variant only has to reach its last checkpoint column)
		const int nsteps = DUMP ? (dlast < 0 ? 0 : (dlast + 1 < n ? dlast + 1 : n) + 127) : n + 127;
		// The step body is instantiated twice per loop iteration: within one step the new H column is written into the
		// registers the profile rows were loaded into (the old H column is still being read), so consecutive steps
		// alternate between two register banks; with a single copy of the body the compiler has to move the whole column
		// back at the end of every step (~16 v_mov_b64 of ~230 instructions).
		// (DRAIN: the ROWS variant's copy of the body for the steps >= n, in which a half may be on a drain column)
		auto do_step = [&](const int step, auto drain_c) __attribute__((always_inline)) {
			constexpr bool DRAIN = decltype(drain_c)::value;
			int rvalid = -1;           // ROWS, DRAIN: 0xFFFF in the halves whose column step - v is a real one (< n)
			if constexpr (ROWS && DRAIN) { const int c_lo = step - 2 * lane; rvalid = (c_lo < n ? 0xFFFF : 0) | (c_lo - 1 < n ? (int)0xFFFF0000u : 0); }
			if ((step & 63) == 0) {
				const int c = step + lane;
				chunk = c < n ? (int)tc_unit[c] : CODE_N;
				if (!first_tile) bchunk = c < n ? bnd[c] : make_uint2(0u, 0u);     // bottom row of the previous tile
			}
			const int newcode = __builtin_amdgcn_readlane(chunk, step & 63);
			// hand-over from virtual lane v-1 (computed one step ago; lane 0 takes zeros or the previous tile's bottom row)
			tc = vshift(tc, newcode << 16);
			int recv_h, recv_f, recv_cm, recv_fp;
			if (first_tile) {
				recv_h = vshift0(hbot); recv_f = vshift0(fbot); recv_cm = vshift0(cm); recv_fp = vshift0(fpo);
			} else {
				const uint32_t bx = (uint32_t)__builtin_amdgcn_readlane((int)bchunk.x, step & 63);
				const uint32_t by = (uint32_t)__builtin_amdgcn_readlane((int)bchunk.y, step & 63);
				recv_h = vshift(hbot, (int)(bx << 16)); recv_f = vshift(fbot, (int)(bx & 0xffff0000u));
				recv_cm = vshift(cm, (int)(by << 16)); recv_fp = vshift(fpo, (int)(by & 0xffff0000u));
			}
			const int t_lo = tc & 0xff, t_hi = (tc >> 16) & 0xff;
			const ProfileRows<RP> rows(pl + t_lo * PROF_CODE_STRIDE, pl + t_hi * PROF_CODE_STRIDE + PROF_HALF);
			const int hdiag0 = recv_h_last;           // H[i0-1][c-1]
			recv_h_last = recv_h;
			v2u f = u_from(recv_f);
			v2u fm = (v2u){ 0, 0 };
			if constexpr (DUMP) fm = u_from(vshift0(fmbot)) & ~startm;      // the main pass starts every stripe with F = 0
			// ROWS: the running maximum of the row takes the new H (DRAIN: of the halves on a real column)
			auto row_hook = [&](int r, int h) __attribute__((always_inline)) { if constexpr (ROWS) rowmax_in_place(RM[r], DRAIN ? (h & rvalid) : h); };
			v2s lmax;
			if constexpr (F16) {
				int ff = recv_f;
				lmax = s_from(f16_row_pair(H, E, hbot, ff, hdiag0, rows, HfGapConst<f16c2(2 * GAP_OPEN), f16c2(2 * GAP_EXT)>(), act, row_hook));
				f = u_from(ff);
			} else {
				const v2u KOPEN = (v2u){ 2 * GAP_OPEN, 2 * GAP_OPEN }, KEXT = (v2u){ 2 * GAP_EXT, 2 * GAP_EXT };
				// DUMP: the reference's own E and the F chain restarted at the top of each stripe
				auto dump_hook = [&](int r, v2s t) __attribute__((always_inline)) {
					if constexpr (DUMP) {
						const v2s hm = __builtin_elementwise_max(__builtin_elementwise_max(t, s_from(Es[r])), as_s(fm));
						const v2u hom = __builtin_elementwise_sub_sat(as_u(hm), KOPEN);
						Es[r] = to_int(__builtin_elementwise_max(__builtin_elementwise_sub_sat(u_from(Es[r]), KEXT), hom));
						const v2u fmn = __builtin_elementwise_max(__builtin_elementwise_sub_sat(fm, KEXT), hom);
						fm = (r == RP - 1) ? ((fmn & actm) | (fm & ~actm)) : fmn;
					}
				};
				lmax = int_row_pair<IntRowPolicy<true, false>>(H, E, hbot, f, hdiag0, rows, KOPEN, KEXT, act, row_hook, dump_hook);
			}
			// pin the reduction here: if the compiler sinks it below the hazard branch, the 22 pre-branch H values stay alive
			// next to the (possibly tainted) ones and the common path pays a register copy per row at the join
			asm volatile("" :: "v"(to_int(lmax)));
			// (F16: the values are non-negative, so their bit patterns order like the values: the running maxima stay u16 maxima)
			if constexpr (!DUMP) ubacc = __builtin_elementwise_max(ubacc, as_u(lmax));
			fbot = to_int(f);
			if constexpr (DUMP) fmbot = to_int(fm);
			// ---- Q2 hazard (q2_rows of systolic.h; values doubled, taint in bit 0) -------------------------------
			fpo = 0;
			// (PAST_CUT: one scalar compare says both "long stripes" and "the cut is not proven yet")
			const bool rows_tracked = PAST_CUT ? step < q2_until : lvl2;
			if (rows_tracked) {
				if (q2_rows<2, F16>(H, E, hbot, fpo, recv_f, recv_fp, startm, actm, act, (v2u){ 0xffff, 0xffff }))
					first_enter = first_enter < step ? first_enter : step;
			} else if (!PAST_CUT || !lvl2) {
				// short stripes (ceil(m/16) < 96): a chain may cross several stripes, the row analysis does not hold; any
				// F[b] >= 132 sends the unit to the stripe-faithful kernel
				hzacc |= __builtin_elementwise_sub_sat(u_from(recv_f), ln.fthr2);
			}
			if constexpr (DUMP) {
				// my lo half has just finished column step - 2*lane, my hi half column step - 2*lane - 1
				const int col_lo = step - 2 * lane, col_hi = col_lo - 1;
				if (__builtin_amdgcn_ballot_w64(col_lo == dnext[0] || col_hi == dnext[1]) != 0ull) {
					if (col_lo == dnext[0]) {
						uint16_t* sp = a.dump_state + (size_t)(item.first + dnx[0]) * 2 * a.rows_total + drow0[0];
#pragma unroll
						for (int r = 0; r < RP; r++) if (r < drows[0]) { sp[r] = (uint16_t)H[r]; sp[a.rows_total + r] = (uint16_t)Es[r]; }
						dnx[0]++;
						dnext[0] = dnx[0] < item.count ? dc[dnx[0]] : 0x7fffffff;
					}
					if (col_hi == dnext[1]) {
						uint16_t* sp = a.dump_state + (size_t)(item.first + dnx[1]) * 2 * a.rows_total + drow0[1];
#pragma unroll
						for (int r = 0; r < RP; r++) if (r < drows[1]) { sp[r] = (uint16_t)((uint32_t)H[r] >> 16); sp[a.rows_total + r] = (uint16_t)((uint32_t)Es[r] >> 16); }
						dnx[1]++;
						dnext[1] = dnx[1] < item.count ? dc[dnx[1]] : 0x7fffffff;
					}
				}
			}
			cm = to_int(__builtin_elementwise_max(__builtin_bit_cast(v2u, recv_cm), as_u(lmax)));
			const int cdone = step - 127;
			if (lane == 63 && cdone >= 0) {
				if (last_tile) out[cdone] = F16 ? (uint16_t)f16_int((uint32_t)cm >> 16) : (uint16_t)((uint32_t)cm >> 16);
				else bnd[cdone] = make_uint2(((uint32_t)hbot >> 16) | ((uint32_t)fbot & 0xffff0000u), ((uint32_t)cm >> 16) | ((uint32_t)fpo & 0xffff0000u));
			}
		};
		int step = DUMP ? item.step0 : 0;
		// pipeline snapshot (every SCAN_SNAP_STEPS steps, all lanes at once: ~50 stores per 1024 steps of ~230 instructions)
		auto take_snapshot = [&]() __attribute__((always_inline)) {
			uint32_t* sp = a.snap + ((size_t)unit * a.snap_per_unit + (step / SCAN_SNAP_STEPS - 1)) * (SNAP_DW * 64) + lane;
			// (F16: the checkpoint pass that reads them is the integer kernel)
			auto sv = [](int x) -> uint32_t { return (uint32_t)(F16 ? hf_to_u16(x) : x); };
#pragma unroll
			for (int r = 0; r < RP; r++) { sp[(2 * r) * 64] = sv(H[r]); sp[(2 * r + 1) * 64] = sv(E[r]); }
			sp[(2 * RP) * 64] = (uint32_t)tc; sp[(2 * RP + 1) * 64] = sv(hbot); sp[(2 * RP + 2) * 64] = sv(fbot); sp[(2 * RP + 3) * 64] = sv(cm);
			sp[(2 * RP + 4) * 64] = sv(recv_h_last); sp[(2 * RP + 5) * 64] = (uint32_t)fpo;
		};
		auto close_block = [&]() __attribute__((always_inline)) {
			if (F16) ovf |= __builtin_amdgcn_ballot_w64(ubacc[0] >= F16_2048 || ubacc[1] >= F16_2048) != 0ull;
			const v2u ub = F16 ? u_from(hf_to_u16(to_int(ubacc))) : ubacc;
			if (a.ublk) a.ublk[(((size_t)unit * a.ntiles + a.tile) * a.ublk_blocks + (step / SCAN_UBLK_STEPS)) * 64 + lane] = ublk_pack(ub);
			if constexpr (PAST_CUT) {
				// a clean (even) maximum >= 2 * 251 in either half: the block ended with step + 1
				if (cut_stops && q2_until == 0x7fffffff) {
					constexpr unsigned CUT2 = 2 * (255 - BIAS);
					if (__builtin_amdgcn_ballot_w64((ub[0] >= CUT2 && !(ub[0] & 1)) || (ub[1] >= CUT2 && !(ub[1] & 1))) != 0ull) q2_until = step + 1 + 128;
				}
			}
			ubacc = (v2u){ 0, 0 };
		};
		// steps come in pairs (a block of SCAN_UBLK_STEPS steps ends after an odd step); the checkpoint pass takes no snapshots and
		// keeps no block maxima
#define FASIM_SCAN_STEPS(LIMIT, DRAIN_C) \
		for (; step + 1 < (LIMIT); step += 2) { \
			if constexpr (!DUMP) { if (a.snap && step != 0 && (step & (SCAN_SNAP_STEPS - 1)) == 0 && step / SCAN_SNAP_STEPS <= a.snap_per_unit) take_snapshot(); } \
			do_step(step, DRAIN_C); do_step(step + 1, DRAIN_C); \
			if constexpr (!DUMP) { if (((step + 1) & (SCAN_UBLK_STEPS - 1)) == SCAN_UBLK_STEPS - 1) close_block(); } \
		}
		// ROWS: the same loop twice: steps [0, n) only see real (or fill) columns, the rest goes through the masking copy of the body
		if constexpr (ROWS) FASIM_SCAN_STEPS(n, std::false_type{})
		FASIM_SCAN_STEPS(nsteps, std::bool_constant<ROWS>{})
#undef FASIM_SCAN_STEPS
		if (step < nsteps) do_step(step, std::bool_constant<ROWS>{});
		if constexpr (!DUMP) {
			// the last, partial block (nsteps - 1 is its last step unless the block was just closed)
			if (a.ublk && (nsteps & (SCAN_UBLK_STEPS - 1)) != 0) a.ublk[(((size_t)unit * a.ntiles + a.tile) * a.ublk_blocks + ((nsteps - 1) / SCAN_UBLK_STEPS)) * 64 + lane] = ublk_pack(F16 ? u_from(hf_to_u16(to_int(ubacc))) : ubacc);
		}
		if constexpr (F16) {
			// (a block that was just closed left ubacc = 0)
			ovf |= __builtin_amdgcn_ballot_w64(ubacc[0] >= F16_2048 || ubacc[1] >= F16_2048) != 0ull;
			if (ovf && lane == 0) a.unit_ovf[unit] = 1;
		}
		if constexpr (ROWS) {
			// every row [0, rows_total) belongs to exactly one half (row0 + rows <= rows_total: lane_rows), which owns RP or RP - 1
			// rows: the transparent last register row of a half that owns RP - 1 (act == 0) is not stored
			uint16_t* rp = a.rowmax16 + (size_t)unit * a.rows_total;
#pragma unroll
			for (int r = 0; r < RP; r++) {
				const uint32_t x = (uint32_t)(F16 ? hf_to_u16(RM[r]) : RM[r]);
				if (r < RP - 1 || (act & 0xFFFFu)) rp[ln.row0[0] + r] = (uint16_t)x;
				if (r < RP - 1 || (act >> 16)) rp[ln.row0[1] + r] = (uint16_t)(x >> 16);
			}
		}
		if (a.unit_hz && __builtin_amdgcn_ballot_w64(to_int(hzacc) != 0) != 0ull && lane == 0) atomicOr(a.unit_hz + unit, 1);
		if (!DUMP && a.unit_first && first_enter != 0x7fffffff && lane == 0) atomicMin(a.unit_first + unit, first_enter);
	}
}

template <int RP>
static hipError_t launch_scan_dump_t(const ScanArgs& a, hipStream_t st)
{
	hipError_t err = hipMemsetAsync(a.counter, 0, sizeof(uint32_t), st);
	if (err != hipSuccess) return err;
	const long blocks = ((long)a.nwork + 3) / 4;              // one work item per wave
	hipLaunchKernelGGL((k_scan<RP, true>), dim3((unsigned)blocks), dim3(256), (size_t)5 * PROF_CODE_STRIDE, st, a);
	return hipGetLastError();
}

template <int RP, bool F16, bool ROWS>
static hipError_t launch_scan_t(const ScanArgs& a, hipStream_t st)
{
	hipError_t err = hipMemsetAsync(a.counter, 0, sizeof(uint32_t), st);
	if (err != hipSuccess) return err;
	// Short-lived workgroups (each wave takes about two units from the queue) instead of a persistent grid: slots free up every
	// few milliseconds, so the latency-bound kernels of the other batches in flight get dispatched at once instead of waiting
	// for this kernel to drain.
	constexpr int WPB = 4, PER_WAVE = 2;                 // waves per workgroup, units per wave
	const long blocks = ((long)a.nwork + WPB * PER_WAVE - 1) / (WPB * PER_WAVE);
	hipLaunchKernelGGL((k_scan<RP, false, F16, ROWS>), dim3((unsigned)blocks), dim3(256), (size_t)5 * PROF_CODE_STRIDE, st, a);
	return hipGetLastError();
}

// virtual lanes per reference stripe for a query of m rows: a multiple of 8 (so that a tile of 128 virtual lanes is
// always full) with at most 24 rows per virtual lane
int systolic_vs(int m) { const int seg = (m + 15) / 16; return 8 * ((seg + 191) / 192); }
int systolic_tiles(int m) { return systolic_vs(m) / 8; }
int systolic_snap_dwords(int m) { const int seg = (m + 15) / 16, vs = systolic_vs(m); return 2 * ((seg + vs - 1) / vs) + 6; }
// (31 tiles hold FASIM_MAX_QUERY = 92 256 rows: seg 5 766, vs 248, RP 24)
bool systolic_fits(int m) { const int seg = (m + 15) / 16; return seg >= 8 && systolic_tiles(m) <= SYSTOLIC_MAX_TILES; }

hipError_t launch_scan(const ScanLaunch& L, hipStream_t st)
{
	if (L.nwork <= 0) return hipSuccess;
	if (!systolic_fits(L.m)) return hipErrorInvalidValue;      // tiny or huge queries: striped kernels
	ScanArgs a;
	a.tcodes = L.tcodes; a.unit_ids = L.unit_ids; a.unit_len = L.unit_len; a.nwork = L.nwork; a.tstride = L.tstride;
	a.counter = L.counter; a.qcodes = L.qcodes; a.m = L.m; a.m_pad = 16 * ((L.m + 15) / 16); a.seg_len16 = (L.m + 15) / 16;
	for (int i = 0; i < 25; i++) a.score[i] = L.score[i];
	a.colmax16 = L.colmax16; a.unit_hz = L.unit_hz; a.coarse = L.coarse;
	a.vs = systolic_vs(L.m); a.ntiles = a.vs / 8; a.boundary = L.boundary;
	a.unit_first = L.unit_first; a.snap = L.snap; a.snap_per_unit = L.snap_per_unit; a.dump_items = L.dump_items; a.dump_cols = L.dump_cols; a.dump_state = L.dump_state; a.rows_total = 16 * a.seg_len16;
	a.ublk = L.dump_items ? nullptr : L.ublk; a.ublk_blocks = L.ublk_blocks;
	const bool f16 = L.f16 && !L.dump_items;
	if (f16 && !L.unit_ovf) return hipErrorInvalidValue;
	a.unit_ovf = L.unit_ovf;
	a.rowmax16 = L.dump_items ? nullptr : L.rowmax16;
	a.q2_past_cut = L.q2_past_cut;
	const bool rows = a.rowmax16 != nullptr;
	if (a.ntiles > 1 && !a.boundary) return hipErrorInvalidValue;
	// RP must be exactly ceil(segLen/vs): every virtual lane then owns RP or RP-1 rows.  One launch per tile of 128
	// virtual lanes (long queries): tile t reads the bottom row tile t-1 left in `boundary` and overwrites it in place.
	const int rp = (a.seg_len16 + a.vs - 1) / a.vs;
	for (int t = 0; t < a.ntiles; t++) {
		a.tile = t;
		hipError_t err = hipErrorInvalidValue;
		switch (rp) {
#define FASIM_SCAN_CASE(N) case N: err = L.dump_items ? launch_scan_dump_t<N>(a, st) : (rows ? (f16 ? launch_scan_t<N, true, true>(a, st) : launch_scan_t<N, false, true>(a, st)) : (f16 ? launch_scan_t<N, true, false>(a, st) : launch_scan_t<N, false, false>(a, st))); break;
		FASIM_SCAN_CASE(1) FASIM_SCAN_CASE(2) FASIM_SCAN_CASE(3) FASIM_SCAN_CASE(4) FASIM_SCAN_CASE(5) FASIM_SCAN_CASE(6)
		FASIM_SCAN_CASE(7) FASIM_SCAN_CASE(8) FASIM_SCAN_CASE(9) FASIM_SCAN_CASE(10) FASIM_SCAN_CASE(11) FASIM_SCAN_CASE(12)
		FASIM_SCAN_CASE(13) FASIM_SCAN_CASE(14) FASIM_SCAN_CASE(15) FASIM_SCAN_CASE(16) FASIM_SCAN_CASE(17) FASIM_SCAN_CASE(18)
		FASIM_SCAN_CASE(19) FASIM_SCAN_CASE(20) FASIM_SCAN_CASE(21) FASIM_SCAN_CASE(22) FASIM_SCAN_CASE(23) FASIM_SCAN_CASE(24)
#undef FASIM_SCAN_CASE
		default: break;
		}
		if (err != hipSuccess) return err;
	}
	return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// k_scan_post: one wave per unit.  Applies the reference's overflow rule (Q1, sswNew.cpp:384-395): the first
// column whose maximum reaches 251 and everything after it is treated as 0; derives the stage-1 score
// (own maximum unless a separate stage-1 pass supplied it), the threshold (int)(score*0.8), the hazard
// flag (a tainted column maximum that is a hit or decides the cut, or the kernel's own unit flag), and the
// ordered list of columns above the threshold.  Input values are 2*max + taint.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_scan_post(const uint16_t* __restrict__ colmax16, const int32_t* __restrict__ unit_ids,
	const int32_t* __restrict__ unit_len, int32_t tstride, const int32_t* __restrict__ stage1_in, uint32_t* __restrict__ hits,
	uint32_t hits_cap, uint32_t* __restrict__ hits_total, int32_t* __restrict__ hit_off, int32_t* __restrict__ hit_cnt,
	int32_t* __restrict__ thr_out, int32_t* __restrict__ stage1_out, int32_t* __restrict__ flags, const int32_t* __restrict__ unit_hz)
{
	const int unit = unit_ids[blockIdx.x];
	const int lane = threadIdx.x;
	const int n = unit_len[unit];
	const uint16_t* col = colmax16 + (int64_t)unit * tstride;
	int mx = 0, cut = n;
	for (int c0 = 0; c0 < n; c0 += 64) {
		const int c = c0 + lane;
		const int v = c < n ? (int)(col[c] >> 1) : 0;
		mx = max(mx, v);
		const unsigned long long over = __ballot(v >= 255 - BIAS);
		if (over && cut == n) cut = c0 + __ffsll((long long)over) - 1;
	}
	for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
	int s1 = mx;
	if (stage1_in && stage1_in[unit] >= 0) s1 = stage1_in[unit];
	const int thr = (int)((double)s1 * 0.8);          // Fasim-LongTarget.cpp:413
	int cnt = 0; bool hz = false;
	for (int c0 = 0; c0 < n; c0 += 64) {
		const int c = c0 + lane;
		const int raw = c < n ? (int)col[c] : 0;
		const int v = raw >> 1;
		if (c <= cut && (raw & 1) && (v > thr || v >= 255 - BIAS)) hz = true;
		const bool hit = c < cut && v > thr;
		cnt += __popcll(__ballot(hit));
	}
	hz = __ballot(hz) != 0ull || (unit_hz && unit_hz[unit] != 0);
	uint32_t off = 0;
	if (lane == 0) off = atomicAdd(hits_total, (uint32_t)cnt);
	off = __shfl(off, 0, 64);
	if (lane == 0) {
		hit_off[unit] = (int32_t)off; hit_cnt[unit] = cnt; thr_out[unit] = thr; stage1_out[unit] = s1;
		flags[unit] = (hz ? 1 : 0) | (cut < n ? 2 : 0) | (mx >= 16383 ? 4 : 0);     // 16383 = saturated 16-bit lanes
	}
	if ((uint64_t)off + (uint64_t)cnt > hits_cap) return;
	uint32_t wpos = off;
	for (int c0 = 0; c0 < n; c0 += 64) {
		const int c = c0 + lane;
		const int v = c < n ? (int)(col[c] >> 1) : 0;
		const bool hit = c < cut && v > thr;
		const unsigned long long b = __ballot(hit);
		if (hit) hits[wpos + __popcll(b & ((1ull << lane) - 1ull))] = ((uint32_t)c << 8) | (uint32_t)v;
		wpos += __popcll(b);
	}
}

hipError_t launch_scan_post(const uint16_t* colmax16, const int32_t* unit_ids, int32_t nwork, const int32_t* unit_len,
	int32_t tstride, const int32_t* stage1_in, uint32_t* hits, uint32_t hits_cap, uint32_t* hits_total, int32_t* hit_off,
	int32_t* hit_cnt, int32_t* thr_out, int32_t* stage1_out, int32_t* flags, const int32_t* unit_hz, hipStream_t st)
{
	if (nwork <= 0) return hipSuccess;
	hipError_t err = hipMemsetAsync(hits_total, 0, sizeof(uint32_t), st);
	if (err != hipSuccess) return err;
	hipLaunchKernelGGL(k_scan_post, dim3((unsigned)nwork), dim3(64), 0, st, colmax16, unit_ids, unit_len, tstride, stage1_in, hits,
		hits_cap, hits_total, hit_off, hit_cnt, thr_out, stage1_out, flags, unit_hz);
	return hipGetLastError();
}

// maximum of the column maxima (stored as 2*max + taint) of each listed unit (used for the separate stage-1 pass of units with N)
__global__ void __launch_bounds__(64) k_max16(const uint16_t* __restrict__ colmax16, const int32_t* __restrict__ unit_ids,
	const int32_t* __restrict__ unit_len, int32_t tstride, int32_t* __restrict__ out)
{
	const int unit = unit_ids[blockIdx.x];
	const int n = unit_len[unit];
	const uint16_t* col = colmax16 + (int64_t)unit * tstride;
	int mx = 0;
	for (int c = threadIdx.x; c < n; c += 64) mx = max(mx, (int)(col[c] >> 1));
	for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
	if (threadIdx.x == 0) out[unit] = mx;
}

hipError_t launch_max16(const uint16_t* colmax16, const int32_t* unit_ids, int32_t nwork, const int32_t* unit_len,
	int32_t tstride, int32_t* out, hipStream_t st)
{
	if (nwork <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_max16, dim3((unsigned)nwork), dim3(64), 0, st, colmax16, unit_ids, unit_len, tstride, out);
	return hipGetLastError();
}

// the instruction the f16 row pair rests on, exposed for the unit test (fasim_maximum3_f16)
__global__ void __launch_bounds__(256) k_maximum3_f16(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
	uint32_t* __restrict__ out3, uint32_t* __restrict__ out0, int64_t n)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	out3[i] = (uint32_t)hf_max3((int)a[i], (int)b[i], (int)c[i]);
	out0[i] = (uint32_t)hf_max_floor((int)a[i], (int)b[i]);
}

hipError_t launch_maximum3_f16(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out3, uint32_t* out0, int64_t n, hipStream_t st)
{
	if (n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_maximum3_f16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, c, out3, out0, n);
	return hipGetLastError();
}

} // namespace fasim
