// fasim-longtarget_amd/csrc/variant_path.hip -- the alignment behind a variant score: the path through the touching matrix T of
// variant.hip, traced in T itself, for gfx950.
//
// An item is one problem of the launch that k_hap_encode and k_touch served (its target codes are still in place) together with the
// plain value its unit attains.  k_touch_path runs k_touch's column step over it once more -- the same ColState, col_row and col_cell
// of colstep.h, uniform loops --, in plain values (the clip bit is dropped), and keeps one direction byte per cell:
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
#include "colstep.h"

namespace fasim {

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
	ColState<NT, IN_LDS> S;
	S.open(tp_lds, lds_rows, a.rows, k, a.qcodes, a.m);
	const int m = a.m, t = S.t, rpt = S.rpt;
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
		const int top = t > 0 ? (int)cur[S.above] : 0;      // H of the previous column in the row above the thread's first
		// first walk: what the thread's own rows hand to the row below them.  A gap never opens better from a cell that a gap reached,
		// so the H of a row may stand without the gap that enters the thread from above
		int hd = top, f = 0, hn = 0;
		for (int i0 = 0; i0 < rpt; i0 += COL_UNROLL) {
			int hc[COL_UNROLL], ein[COL_UNROLL], sc[COL_UNROLL];
#pragma unroll
			for (int u = 0; u < COL_UNROLL; u++) col_row<1>(S, cur, min(i0 + u, rpt - 1), tcode, hc[u], ein[u], sc[u]);
#pragma unroll
			for (int u = 0; u < COL_UNROLL; u++) if (i0 + u < rpt) {
				int e;
				hn = col_cell<1>(hd, hc[u], ein[u], sc[u], cont, i0 + u > 0, hn, f, e);
				hd = hc[u];
			}
		}
		const int fin = col_gap_in<1>(S, col_gap<1>(f, hn), wtot);
		// second walk: the recurrence itself, with the direction byte of every cell
		int hit = 0, hrow = 0x7fffffff;
		hd = top; f = fin; hn = 0;
		const int cbase = c * rpt;
		for (int i0 = 0; i0 < rpt; i0 += COL_UNROLL) {
			int hc[COL_UNROLL], ein[COL_UNROLL], sc[COL_UNROLL];
#pragma unroll
			for (int u = 0; u < COL_UNROLL; u++) col_row<1>(S, cur, min(i0 + u, rpt - 1), tcode, hc[u], ein[u], sc[u]);
#pragma unroll
			for (int u = 0; u < COL_UNROLL; u++) if (i0 + u < rpt) {
				int e;
				const int h = col_cell<1>(hd, hc[u], ein[u], sc[u], cont, i0 + u > 0, hn, f, e);
				const int src = (hd > 0 && h == hd + sc[u]) ? 0 : ((hd == 0 && !cont && h == sc[u]) ? 1 : (h == e ? 2 : 3));
				dirs[(cbase + i0 + u) * NT + t] = (uint8_t)(src | ((e == ein[u] - 4) ? 4 : 0) | ((f - 4 >= h - 16) ? 8 : 0));
				if (counts && i0 + u < S.cnt && h == value && !hit) { hit = 1; hrow = S.first + i0 + u; }
				nxt[S.at(i0 + u)] = (uint16_t)h; S.e[S.at(i0 + u)] = (uint16_t)e;
				hd = hc[u]; hn = h;
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
		CigarRun cig(a.cigar + I.cig_off, I.cig_cap);
		int i = hit_row, j = jend, state = 0;
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
			if (!cig.push(op)) { bad = true; break; }
		}
		if (!done) bad = true;
		if (!bad && !cig.flush()) bad = true;
		len = bad ? -1 : cig.nops;
	}
	TouchPathOut O;
	O.i1 = i1; O.j1 = j1; O.i0 = ia; O.j0 = ja; O.cigar_len = len; O.pad[0] = O.pad[1] = O.pad[2] = 0;
	a.out[k] = O;
}

hipError_t launch_touch_path(const TouchPathLaunch& L, hipStream_t st)
{
	if (L.nitem <= 0) return hipSuccess;
	if (L.m < 1 || !L.tcodes || !L.qcodes || !L.probs || !L.items || !L.dirs || !L.cigar || !L.out) return hipErrorInvalidValue;
	return launch_cols(L, L.nitem, st, [](auto nt, auto lds) { return k_touch_path<decltype(nt)::value, decltype(lds)::value>; });
}

} // namespace fasim
