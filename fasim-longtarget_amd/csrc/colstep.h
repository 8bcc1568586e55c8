// fasim-longtarget_amd/csrc/colstep.h -- the column-parallel Gotoh step shared by k_site_ends / k_site_path (site_align.hip), k_touch
// (variant.hip) and k_touch_path (variant_path.hip) for gfx950.
//
// The step: one workgroup per problem, a thread owns a block of query rows, and a column is a walk of the thread's rows, an
// exclusive max-scan of the vertical gap value the thread hands to the row below its last, and a second walk that takes in the gap
// that enters from above.  A gap never opens better from a cell that a gap reached, so the first walk may open gaps from its own H.
// What a kernel gets from this header: NEG32 and scan_excl (all four kernels); ColState, col_row / col_load, col_cell and col_gap_in (the two
// touch kernels, which must stay cell-for-cell equal: k_touch_path traces the very matrix k_touch scored); CigarRun (the two
// tracebacks); lds_bytes and launch_cols (the launchers).  What a kernel keeps: its walks around the cell (mark, best, direction
// byte, hit test, what is stored), its barriers and its traceback.  sa_pass (site_align.hip) keeps its contiguous row layout, its
// signed state and its three modes, and takes only the scan.  Everything here is __device__ __forceinline__, constexpr or host inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "kernels.h"

namespace fasim {

constexpr int NEG32 = -(1 << 28);              // "nothing handed down" in the scan

// exclusive max-scan of b over the NT threads of the workgroup (thread order); wtot: one word of LDS per wave.  Contains one
// __syncthreads where the workgroup has more than one wave.
template <int NT>
__device__ __forceinline__ int scan_excl(int b, int* wtot, int lane, int wave)
{
	int inc = b;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int x = __shfl_up(inc, d);
		if (lane >= d) inc = max(inc, x);
	}
	int ex = __shfl_up(inc, 1);
	if (lane == 0) ex = NEG32;
	if (NT > 64) {
		if (lane == 63) wtot[wave] = inc;
		__syncthreads();
		for (int w = 0; w < wave; w++) ex = max(ex, wtot[w]);
	}
	return ex;
}

// ---- the cell, in values times SCALE ------------------------------------------------------------------------------------------------
// SCALE 1: plain values, +5 / -4, gap 16 then 4, floor at 0.  SCALE 2: k_touch's 2 * value + clip bit, +10 / -8, gap 32 then 8; a
// lone bit is value 0: no alignment, no bit.  The bit travels through every maximum and every add; setting it is the caller's.
template <int SCALE> __device__ __forceinline__ int col_score(int qc, int tc) { return (qc == tc && tc < 4) ? 5 * SCALE : -4 * SCALE; }
template <int SCALE> __device__ __forceinline__ int col_floor(int x) { return SCALE == 2 ? (x < 2 ? 0 : x) : max(x, 0); }
// the gap value a row with gap value g and H h hands to the next row (vertical) or column (horizontal), before the floor
template <int SCALE> __device__ __forceinline__ int col_gap(int g, int h) { return max(g - 4 * SCALE, h - 16 * SCALE); }

// One cell of the touching matrix: hd = H of the previous column in the row above, hc / ein = H and E of the previous column in this
// row, sc = the pair's score, f / hn = F and H of the row above in this column (below: there is one in this walk).  cont: the column
// lies behind the allele, where the diagonal only continues an alignment.  Returns H; e and f are this row's.
template <int SCALE>
__device__ __forceinline__ int col_cell(int hd, int hc, int ein, int sc, bool cont, bool below, int hn, int& f, int& e)
{
	e = col_floor<SCALE>(col_gap<SCALE>(ein, hc));
	if (below) f = col_floor<SCALE>(col_gap<SCALE>(f, hn));
	int dg = hd + sc;
	if (cont) dg = hd ? dg : 0;
	const int de = max(dg, e);                   // (plain values: e >= 0 floors it)
	return max(SCALE == 2 ? col_floor<SCALE>(de) : de, f);
}

// ---- the strided row state of the touch kernels -------------------------------------------------------------------------------------
// One workgroup of NT threads per problem (NT = 64 or 128 for queries of at most that many rows, else 256).  Thread t owns rows
// [t * rpt, (t + 1) * rpt); the state of its i-th row (H of the previous column, H of this column, E: 16-bit, unsigned) lives at
// [i * NT + t], so that the lanes of a wave read and write neighbouring 16-bit words (no LDS bank conflicts, coalesced in HBM).
// IN_LDS: dynamic LDS of [lds_rows] x (3 x uint16 + 1 code byte), lds_rows = rpt * NT (every pointer of the column step is then an LDS
// pointer at compile time: ds_read_u16, not a flat load); otherwise the row state lives in HBM and the codes are read from there.
// Every thread walks rpt rows: the rows from m on (the last rows of the last threads) lie below every real row, so nothing of them
// reaches a real cell; the caller only keeps them out of its results (i < cnt).
template <int NT, bool IN_LDS>
struct ColState {
	uint16_t* h[2];                             // [rows]: H of the previous / this column, swapped every column
	uint16_t* e;                                // [rows]
	const uint8_t* q;                           // query codes (LDS copy or HBM): the code of the thread's i-th row is q[q0 + min(i, qlast) * qstep]
	int t, rpt, first, cnt;                     // the thread, rows per thread, its first row and how many of its rows are real
	int qstep, q0, qlast;
	int above;                                  // index of the last row of the thread before this one

	__device__ __forceinline__ int at(int i) const { return i * NT + t; }
	// lds: the workgroup's dynamic LDS; rows: the launch's HBM row state, `block` this workgroup's slot in it.  Zero-fills H and E;
	// the caller's __syncthreads follows.
	__device__ __forceinline__ void open(unsigned char* lds, int lds_rows, uint16_t* rows, int64_t block, const uint8_t* qcodes, int m)
	{
		t = threadIdx.x; rpt = (m + NT - 1) / NT;
		first = min(m, t * rpt); cnt = min(m, first + rpt) - first;
		if (IN_LDS) {
			uint16_t* b = reinterpret_cast<uint16_t*>(lds);
			h[0] = b; h[1] = b + lds_rows; e = b + 2 * lds_rows;
			uint8_t* qc = reinterpret_cast<uint8_t*>(b + 3 * lds_rows);
			for (int i = 0; i < rpt; i++) qc[at(i)] = i < cnt ? qcodes[first + i] : 4;
			q = qc;
		} else {
			uint16_t* b = rows + block * 3 * rpt * NT;
			h[0] = b; h[1] = b + rpt * NT; e = b + 2 * rpt * NT;
			q = qcodes;
		}
		qstep = IN_LDS ? NT : 1; q0 = IN_LDS ? t : min(first, m - 1); qlast = IN_LDS ? rpt - 1 : m - 1 - q0;
		above = (rpt - 1) * NT + t - 1;
		for (int i = 0; i < rpt; i++) { h[0][at(i)] = 0; e[at(i)] = 0; }
	}
};

constexpr int COL_UNROLL = 4;                  // rows whose state a walk loads ahead of their cells (i = min(i0 + k, rpt - 1): the loads of a
                                               // short last group repeat its last row, no branch around a load)
// H and E of the previous column in the thread's i-th row and the score of its pair
template <int SCALE, int NT, bool IN_LDS>
__device__ __forceinline__ void col_row(const ColState<NT, IN_LDS>& S, const uint16_t* cur, int i, int tcode, int& hc, int& ein, int& sc)
{
	hc = cur[S.at(i)]; ein = S.e[S.at(i)]; sc = col_score<SCALE>(S.q[S.q0 + min(i, S.qlast) * S.qstep], tcode);
}
// ... of the group of rows from i0 on.  k_touch_path writes this loop out: through col_load its HBM build spills SGPRs
// (profiles/r21_colstep_isa.txt)
template <int SCALE, int NT, bool IN_LDS>
__device__ __forceinline__ void col_load(const ColState<NT, IN_LDS>& S, const uint16_t* cur, int i0, int tcode, int (&hc)[COL_UNROLL],
	int (&ein)[COL_UNROLL], int (&sc)[COL_UNROLL])
{
#pragma unroll
	for (int k = 0; k < COL_UNROLL; k++) col_row<SCALE>(S, cur, min(i0 + k, S.rpt - 1), tcode, hc[k], ein[k], sc[k]);
}

// the gap value that enters the thread's first row, from what every thread's rows hand down (out = col_gap of its last row):
//   max over t' < t of out(t') - 4 * SCALE * rpt * (t - 1 - t'), floored.  Contains scan_excl's barrier.
template <int SCALE, int NT, bool IN_LDS>
__device__ __forceinline__ int col_gap_in(const ColState<NT, IN_LDS>& S, int out, int* wtot)
{
	const int ex = scan_excl<NT>(out + 4 * SCALE * S.rpt * S.t, wtot, S.t & 63, S.t >> 6);
	return S.t == 0 ? 0 : col_floor<SCALE>(max(ex, NEG32) - 4 * SCALE * S.rpt * (S.t - 1));
}

// ---- the CIGAR of a traceback, by one lane ------------------------------------------------------------------------------------------
// Runs of equal operations as (length << 4 | op) words, in the order they are pushed: the last operation of the alignment first.
struct CigarRun {
	uint32_t* cig; int cap, nops, run_op, run;
	__device__ __forceinline__ CigarRun(uint32_t* words, int cap_words) : cig(words), cap(cap_words), nops(0), run_op(0), run(0) {}
	// the pending run out; false: the words are full
	__device__ __forceinline__ bool flush()
	{
		if (run == 0) return true;
		if (nops >= cap) return false;
		cig[nops++] = ((uint32_t)run << 4) | (uint32_t)run_op; run = 0;
		return true;
	}
	__device__ __forceinline__ bool push(int op)
	{
		if (op != run_op && !flush()) return false;
		run_op = op; run++;
		return true;
	}
};

// ---- host: LDS size and the dispatch over the workgroup size ------------------------------------------------------------------------
inline size_t lds_bytes(int rows) { return (size_t)rows * 7 + 16; }      // three 16-bit words and a code byte per row

// Launches kernel(NT, IN_LDS)'s instantiation for a launch struct L of the touch kernels (L.m, L.rows): NT by touch_threads(m), the
// row state in LDS up to TOUCH_LDS_ROWS rows.  kernel: a generic lambda from two integral constants to the __global__ function.
template <class Launch, class Kernel>
hipError_t launch_cols(const Launch& L, int nblock, hipStream_t st, Kernel kernel)
{
	const bool lds = L.m <= TOUCH_LDS_ROWS;
	if (!lds && !L.rows) return hipErrorInvalidValue;
	const int nt = touch_threads(L.m), lds_rows = lds ? touch_state_rows(L.m) : 0;
	auto go = [&](auto NT, auto IN_LDS) {
		hipLaunchKernelGGL(kernel(NT, IN_LDS), dim3((unsigned)nblock), dim3(NT.value), lds ? lds_bytes(lds_rows) : 0, st, L, lds_rows);
	};
	if (!lds) go(std::integral_constant<int, 256>(), std::false_type());
	else if (nt == 64) go(std::integral_constant<int, 64>(), std::true_type());
	else if (nt == 128) go(std::integral_constant<int, 128>(), std::true_type());
	else go(std::integral_constant<int, 256>(), std::true_type());
	return hipGetLastError();
}

} // namespace fasim
