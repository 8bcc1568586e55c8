// fasim-longtarget_amd/csrc/variant_path.hip -- the alignment behind a variant score: the path through the touching matrix T of
// variant.hip, traced in T itself, for gfx950.
//
// An item is one problem of the launch that k_var_encode and k_touch served (its target codes are still in place) together with the
// plain value its unit attains.  k_touch_path runs k_touch's column step over it once more -- same workgroup sizes, same row layout
// ([i * NT + t], 16-bit, in LDS or in HBM), same select behind the allele, uniform loops --, in plain values (the clip bit is dropped:
// +5 / -4, gap 16 then 4), and keeps one direction byte per cell:
//     bits 0-1  where H came from: 0 the diagonal (Hdiag > 0), 1 a first pair (Hdiag == 0, before v1), 2 E, 3 F
//     bit 2     E of this cell extends E of the cell to its left (else it opens from H there)
//     bit 3     F of the cell BELOW extends F of this cell (else it opens from H here)
// Bit 3 sits with the cell the gap comes from, not with the cell it enters: every thread then decides it from the final F and H of
// its own rows, and the gap that enters a thread's first row needs no fold over the threads before it.
// The byte of row i of thread t in column c is dirs[(c * rpt + i) * NT + t]: a wave writes neighbouring bytes.
// The first walk of a column only works out what the thread's rows hand down (nothing is stored); after the scan the second walk is
// the recurrence itself.  The pass stops at the first column from v0 on in which a real row holds the value (__syncthreads_or; the
// smallest row by one LDS atomicMin); then one lane walks the bytes back from that cell and writes the CIGAR, last operation first.
// No atomics on global memory, plain vector stores only; every output word and every direction byte has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

constexpr int TP_THREADS = 256;
constexpr int TP_NEG32 = -(1 << 28);           // "nothing handed down" in the scan
constexpr int TP_UNROLL = 4;                   // rows whose state is loaded ahead of their cells

struct TpState {
	uint16_t* h[2];                             // [rows]: H of the previous / this column, swapped every column
	uint16_t* e;                                // [rows]
	const uint8_t* q;                           // query codes (LDS copy or HBM)
};

__device__ __forceinline__ int tp_score(int qc, int tc) { return (qc == tc && tc < 4) ? 5 : -4; }

// exclusive max-scan of b over the NT threads of the workgroup (thread order); wtot: one word of LDS per wave.  Contains one
// __syncthreads where the workgroup has more than one wave.
template <int NT>
__device__ __forceinline__ int tp_scan_excl(int b, int* wtot, int lane, int wave)
{
	int inc = b;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int x = __shfl_up(inc, d);
		if (lane >= d) inc = max(inc, x);
	}
	int ex = __shfl_up(inc, 1);
	if (lane == 0) ex = TP_NEG32;
	if (NT > 64) {
		if (lane == 63) wtot[wave] = inc;
		__syncthreads();
		for (int w = 0; w < wave; w++) ex = max(ex, wtot[w]);
	}
	return ex;
}

// One workgroup of NT threads per item (NT by touch_threads(m)); rows and LDS as in k_touch
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_touch_path(TouchPathLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char tp_lds[];
	__shared__ int wtot[4];
	__shared__ int hit_row;
	const int k = blockIdx.x;
	if (k >= a.nitem) return;
	const TouchPathItem I = a.items[k];
	const TouchProb P = a.probs[I.prob];
	const int m = a.m, t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int rpt = (m + NT - 1) / NT;
	const int first = min(m, t * rpt), cnt = min(m, first + rpt) - first;
	TpState S;
	if (IN_LDS) {
		uint16_t* b = reinterpret_cast<uint16_t*>(tp_lds);
		S.h[0] = b; S.h[1] = b + lds_rows; S.e = b + 2 * lds_rows;
		uint8_t* qc = reinterpret_cast<uint8_t*>(b + 3 * lds_rows);
		for (int i = 0; i < rpt; i++) qc[i * NT + t] = i < cnt ? a.qcodes[first + i] : 4;
		S.q = qc;
	} else {
		uint16_t* b = a.rows + (int64_t)k * 3 * rpt * NT;
		S.h[0] = b; S.h[1] = b + rpt * NT; S.e = b + 2 * rpt * NT;
		S.q = a.qcodes;
	}
	// (the code of the thread's i-th row: S.q[q0 + i * qstep]; rows from m on lie below every real row and only fill the walk)
	const int qstep = IN_LDS ? NT : 1, q0 = IN_LDS ? t : min(first, m - 1), qlast = IN_LDS ? rpt - 1 : m - 1 - q0;
	const int above = (rpt - 1) * NT + t - 1;                                      // the last row of the thread before this one
	for (int i = 0; i < rpt; i++) { S.h[0][i * NT + t] = 0; S.e[i * NT + t] = 0; }
	if (t == 0) hit_row = 0x7fffffff;
	__syncthreads();
	// (uniform) the host sized the direction bytes for n columns of rpt * NT rows, and they are indexed in 32 bits
	const bool ok = P.n >= 1 && P.n <= TOUCH_MAX_COLS && P.v0 >= 0 && P.v0 < P.v1 && P.v1 <= P.n && I.value >= 1 && I.cig_cap >= 1 &&
		(int64_t)P.n * rpt * NT < ((int64_t)1 << 31);
	const uint8_t* tc = a.tcodes + P.tbase;
	uint8_t* dirs = a.dirs + I.dir_off;
	const int value = I.value;
	int jend = -1;
	for (int c = 0; ok && c < P.n; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const int tcode = tc[c];
		const bool cont = c >= P.v1;                 // behind the allele the diagonal only continues an alignment
		const bool counts = c >= P.v0;
		const int top = t > 0 ? (int)cur[above] : 0;      // H of the previous column in the row above the thread's first
		// first walk: what the thread's own rows hand to the row below them.  A gap never opens better from a cell that a gap reached,
		// so the H of a row may stand without the gap that enters the thread from above
		int out;
		{
			int hd = top, f = 0, hn = 0;
			for (int i0 = 0; i0 < rpt; i0 += TP_UNROLL) {
				int hc[TP_UNROLL], ein[TP_UNROLL], sc[TP_UNROLL];
#pragma unroll
				for (int u = 0; u < TP_UNROLL; u++) {      // (the loads of a short last group repeat its last row: no branch around a load)
					const int i = min(i0 + u, rpt - 1);
					hc[u] = cur[i * NT + t]; ein[u] = S.e[i * NT + t]; sc[u] = tp_score(S.q[q0 + min(i, qlast) * qstep], tcode);
				}
#pragma unroll
				for (int u = 0; u < TP_UNROLL; u++) if (i0 + u < rpt) {
					const int e = max(max(ein[u] - 4, hc[u] - 16), 0);
					if (i0 + u > 0) f = max(max(f - 4, hn - 16), 0);
					int dg = hd + sc[u];
					if (cont) dg = hd ? dg : 0;
					hn = max(max(dg, e), f);
					hd = hc[u];
				}
			}
			out = max(f - 4, hn - 16);
		}
		const int ex = tp_scan_excl<NT>(out + 4 * rpt * t, wtot, lane, wave);
		const int fin = t == 0 ? 0 : max(max(ex, TP_NEG32) - 4 * rpt * (t - 1), 0);
		// second walk: the recurrence itself, with the direction byte of every cell
		int hit = 0, hrow = 0x7fffffff;
		{
			int hd = top, f = fin, hn = 0;
			const int cbase = c * rpt;
			for (int i0 = 0; i0 < rpt; i0 += TP_UNROLL) {
				int hc[TP_UNROLL], ein[TP_UNROLL], sc[TP_UNROLL];
#pragma unroll
				for (int u = 0; u < TP_UNROLL; u++) {
					const int i = min(i0 + u, rpt - 1);
					hc[u] = cur[i * NT + t]; ein[u] = S.e[i * NT + t]; sc[u] = tp_score(S.q[q0 + min(i, qlast) * qstep], tcode);
				}
#pragma unroll
				for (int u = 0; u < TP_UNROLL; u++) if (i0 + u < rpt) {
					const int e = max(max(ein[u] - 4, hc[u] - 16), 0);
					if (i0 + u > 0) f = max(max(f - 4, hn - 16), 0);
					int dg = hd + sc[u];
					if (cont) dg = hd ? dg : 0;
					const int h = max(max(dg, e), f);
					const int src = (hd > 0 && h == hd + sc[u]) ? 0 : ((hd == 0 && !cont && h == sc[u]) ? 1 : (h == e ? 2 : 3));
					dirs[(cbase + i0 + u) * NT + t] = (uint8_t)(src | ((e == ein[u] - 4) ? 4 : 0) | ((f - 4 >= h - 16) ? 8 : 0));
					if (counts && i0 + u < cnt && h == value && !hit) { hit = 1; hrow = first + i0 + u; }
					nxt[(i0 + u) * NT + t] = (uint16_t)h; S.e[(i0 + u) * NT + t] = (uint16_t)e;
					hd = hc[u]; hn = h;
				}
			}
		}
		if (__syncthreads_or(hit)) {      // (the column's barrier as well)
			if (hit) atomicMin(&hit_row, hrow);      // (LDS)
			jend = c;
			break;
		}
	}
	__syncthreads();
	if (t != 0) return;
	// traceback by one lane (the direction bytes of the workgroup are visible after the barrier)
	int i1 = -1, j1 = -1, ia = -1, ja = -1, len = -1;
	if (jend >= 0) {
		uint32_t* cig = a.cigar + I.cig_off;
		int i = hit_row, j = jend, state = 0, nops = 0, run_op = 0, run = 0;
		i1 = i; j1 = j;
		bool bad = false, done = false;
		const int limit = 2 * (m + P.n) + 4;
		for (int step = 0; step < limit && !done; step++) {
			if (i < 0 || j < 0 || i >= m) { bad = true; break; }
			const int d = dirs[(j * rpt + i % rpt) * NT + i / rpt];
			int op;
			if (state == 0) {
				const int src = d & 3;
				if (src == 2) { state = 1; continue; }
				if (src == 3) { state = 2; continue; }
				op = 0;
				if (src == 1) { ia = i; ja = j; done = true; }
				else { i--; j--; }
			} else if (state == 1) { op = 2; if (!(d & 4)) state = 0; j--; }
			else {
				if (i < 1) { bad = true; break; }
				op = 1;
				if (!(dirs[(j * rpt + (i - 1) % rpt) * NT + (i - 1) / rpt] & 8)) state = 0;
				i--;
			}
			if (run > 0 && op != run_op) {
				if (nops >= I.cig_cap) { bad = true; break; }
				cig[nops++] = ((uint32_t)run << 4) | (uint32_t)run_op; run = 0;
			}
			run_op = op; run++;
		}
		if (!done) bad = true;
		if (!bad && run > 0) { if (nops >= I.cig_cap) bad = true; else cig[nops++] = ((uint32_t)run << 4) | (uint32_t)run_op; }
		len = bad ? -1 : nops;
	}
	TouchPathOut O;
	O.i1 = i1; O.j1 = j1; O.i0 = ia; O.j0 = ja; O.cigar_len = len; O.pad[0] = O.pad[1] = O.pad[2] = 0;
	a.out[k] = O;
}

static size_t tp_lds_bytes(int rows) { return (size_t)rows * 7 + 16; }

hipError_t launch_touch_path(const TouchPathLaunch& L, hipStream_t st)
{
	if (L.nitem <= 0) return hipSuccess;
	if (L.m < 1 || !L.tcodes || !L.qcodes || !L.probs || !L.items || !L.dirs || !L.cigar || !L.out) return hipErrorInvalidValue;
	const bool lds = L.m <= TOUCH_LDS_ROWS;
	if (!lds && !L.rows) return hipErrorInvalidValue;
	const int nt = touch_threads(L.m);
	const int lds_rows = lds ? touch_state_rows(L.m) : 0;
	const dim3 grid((unsigned)L.nitem);
	if (!lds) hipLaunchKernelGGL((k_touch_path<TP_THREADS, false>), grid, dim3(TP_THREADS), 0, st, L, 0);
	else if (nt == 64) hipLaunchKernelGGL((k_touch_path<64, true>), grid, dim3(64), tp_lds_bytes(lds_rows), st, L, lds_rows);
	else if (nt == 128) hipLaunchKernelGGL((k_touch_path<128, true>), grid, dim3(128), tp_lds_bytes(lds_rows), st, L, lds_rows);
	else hipLaunchKernelGGL((k_touch_path<TP_THREADS, true>), grid, dim3(TP_THREADS), tp_lds_bytes(lds_rows), st, L, lds_rows);
	return hipGetLastError();
}

} // namespace fasim
