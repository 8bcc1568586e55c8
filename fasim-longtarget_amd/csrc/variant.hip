// fasim-longtarget_amd/csrc/variant.hip -- the triplex potential through a variant: per allele window and encoding the best local
// alignment that touches the allele's columns, for gfx950.
//
// A problem is one allele window (flank, allele, flank) under one encoding: n <= TOUCH_MAX_COLS target codes and the allele's columns
// [v0, v1).  k_touch runs the touching matrix T over all m real rows of the query: the plain local Gotoh recurrence of section 11 in
// the columns before v1, and from v1 on the same recurrence with a diagonal that only continues (Hdiag > 0 ? Hdiag + s : 0), so that
// nothing starts afresh behind the allele.  The result is the maximum of T over the columns from v0 on.  Every value is carried as
// 2 * value + b (scores and gap costs doubled): b, the clip bit, is set on the positive cells of a first or last column that the flank
// cut and travels through every maximum and every add; 0 means "no alignment" and carries no bit.
//
// The column step is colstep.h's, in doubled values: one workgroup of touch_threads(m) threads per problem, the 16-bit row state in
// LDS or, for queries above TOUCH_LDS_ROWS rows, in HBM; the arithmetic is 32-bit.
// k_hap_encode (haplotype.hip) assembles and encodes the windows on the device; k_touch_reduce folds the problems of a variant into
// nine words.  No atomics on global memory, plain vector stores only; every output word has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "colstep.h"

namespace fasim {

constexpr int VT_THREADS = 256;

// One workgroup of NT threads per problem; rows, LDS and IN_LDS as ColState has them
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_touch(TouchLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char vt_lds[];
	__shared__ int wtot[4];
	__shared__ unsigned best_sh;
	const int p = blockIdx.x;
	if (p >= a.nprob) return;
	const TouchProb P = a.probs[p];
	ColState<NT, IN_LDS> S;
	S.open(vt_lds, lds_rows, a.rows, p, a.qcodes, a.m);
	const int t = S.t, rpt = S.rpt;
	if (t == 0) best_sh = 0;
	__syncthreads();
	const bool ok = P.n >= 1 && P.n <= TOUCH_MAX_COLS && P.v0 >= 0 && P.v0 < P.v1 && P.v1 <= P.n;      // (uniform)
	const uint8_t* tc = a.tcodes + P.tbase;
	int best = 0;
	for (int c = 0; ok && c < P.n; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const int tcode = tc[c];
		const bool cont = c >= P.v1;                 // behind the allele the diagonal only continues an alignment
		const int mark = ((c == 0 && (P.edge & 1)) || (c == P.n - 1 && (P.edge & 2))) ? 1 : 0;
		const int top = t > 0 ? (int)cur[S.above] : 0;      // H of the previous column in the row above the thread's first
		// first walk: E, and H with the vertical gaps that open in the thread's own rows (hl); what these rows hand to the row below
		// them.  A gap never opens better from a cell that a gap reached (h - 32 < f - 8 where h = f), so the gap value of a row is
		// max(f - 8, h - 32) whichever h, the final one or hl, stands in it.
		const bool counts = c >= P.v0;
		int hd = top, f = 0, hn = 0;
		for (int i0 = 0; i0 < rpt; i0 += COL_UNROLL) {
			int hc[COL_UNROLL], ein[COL_UNROLL], sc[COL_UNROLL];
			col_load<2>(S, cur, i0, tcode, hc, ein, sc);
#pragma unroll
			for (int k = 0; k < COL_UNROLL; k++) if (i0 + k < rpt) {
				int e, h = col_cell<2>(hd, hc[k], ein[k], sc[k], cont, i0 + k > 0, hn, f, e);
				if (mark && h) h |= 1;
				if (counts && i0 + k < S.cnt) best = max(best, h);
				nxt[S.at(i0 + k)] = (uint16_t)h; S.e[S.at(i0 + k)] = (uint16_t)e;
				hd = hc[k]; hn = h;
			}
		}
		const int fin = col_gap_in<2>(S, col_gap<2>(f, hn), wtot);
		// second walk, where a gap enters a thread of the wave from above: H = max(hl, the gap continued from fin)
		if (__any(fin > 0)) {
			f = fin;
			for (int i = 0; i < rpt; i++) {
				if (i > 0) f = col_floor<2>(col_gap<2>(f, hn));
				const int h = max((int)nxt[S.at(i)], f);      // (f carries the bit of the marked cell it comes from)
				if (counts && i < S.cnt) best = max(best, h);
				nxt[S.at(i)] = (uint16_t)h;
				hn = h;
			}
		}
		__syncthreads();
	}
	if (best) atomicMax(&best_sh, (unsigned)best);      // (LDS)
	__syncthreads();
	if (t == 0) a.out[p] = best_sh;
}

__device__ __forceinline__ int vt_class(int enc) { return enc < 12 ? (enc & 1) : (((enc - 12) & 1) ? 3 : 2); }

// one thread per variant of the launch
__global__ void __launch_bounds__(VT_THREADS) k_touch_reduce(TouchReduceLaunch a)
{
	const int v = blockIdx.x * VT_THREADS + threadIdx.x;
	if (v >= a.nvar) return;
	unsigned top = 0;
	for (int al = 0; al < 2; al++) {
		const uint32_t* x = a.touch + ((int64_t)v * 2 + al) * a.nenc;
		for (int cls = 0; cls < 4; cls++) {
			unsigned bx = 0, be = 0xff;
			for (int k = 0; k < a.nenc; k++) {
				if (vt_class(a.enc[k]) != cls) continue;
				const unsigned w = x[k];
				if ((w >> 1) > (bx >> 1)) be = a.enc[k];      // (the encodings come in ascending order)
				bx = max(bx, w);
			}
			top = max(top, bx);
			a.out[(int64_t)v * 9 + al * 4 + cls] = (bx << 8) | be;
		}
	}
	a.out[(int64_t)v * 9 + 8] = top & 1;
}

int touch_threads(int m) { return m <= 64 ? 64 : (m <= 128 ? 128 : VT_THREADS); }
int touch_state_rows(int m) { const int nt = touch_threads(m); return (m + nt - 1) / nt * nt; }

hipError_t launch_touch(const TouchLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (L.m < 1 || !L.tcodes || !L.qcodes || !L.probs || !L.out) return hipErrorInvalidValue;
	return launch_cols(L, L.nprob, st, [](auto nt, auto lds) { return k_touch<decltype(nt)::value, decltype(lds)::value>; });
}

hipError_t launch_touch_reduce(const TouchReduceLaunch& L, hipStream_t st)
{
	if (L.nvar <= 0) return hipSuccess;
	if (!L.touch || !L.out || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_touch_reduce, dim3((unsigned)((L.nvar + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
