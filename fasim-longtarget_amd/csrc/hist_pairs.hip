// fasim-longtarget_amd/csrc/hist_pairs.hip -- k_hist_pairs: k_hist (hist.hip) with the pairs of neighbouring positions counted beside the
// positions, for gfx950.
//
// The number of maximal runs of positions with P >= v is the number of positions with P >= v minus the number of pairs (x - 1, x) with
// min(P[x - 1], P[x]) >= v, so a second histogram, of the pairs' minima, gives the sites of every threshold at once.  The kernel is a
// sibling of k_hist in a file of its own, so that hist.hip compiles to what it compiled to before.  Same front half (class_fold.h),
// same launch shape: one 256-thread workgroup per slice of TRACK_CHUNK positions, a lane owns 8 consecutive positions.
//   * the four values of the position before a lane's first come from the lane before it (__shfl_up on two packed words) and, across a
//     wave boundary, through two LDS words per wave; there is no second fold.  The words live in slots TRACK_CHUNK .. TRACK_CHUNK + 3
//     of the mirror's row `wave`: ClassFold::load never writes them, and value() reads them only in lane 255, which has no position
//     and returns before it reads.  An array of its own would take the workgroup past 32 768 bytes and the CU from five to four;
//   * a pair is counted here when both positions lie outside the zones and in this slice.  The pairs across a slice border and
//     across a zone border are the host's: it gets the first and last values of every slice (border[][][2][4]), and the zones
//     one position longer on their interior side (HistPairsLaunch, kernels.h);
//   * two LDS histograms of 4 x HIST_PAIR_LDS_BINS counters, 16 KB together; larger values go to HBM at once, as in k_hist;
//   * every non-atomic output word has one writer: a zone slot and a border word belong to one position, a position to one lane;
//   * sums of integers do not depend on their order: the result is the same bit for bit on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "class_fold.h"

namespace fasim {

__global__ void __launch_bounds__(256) k_hist_pairs(HistPairsLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t bins[2][4][HIST_PAIR_LDS_BINS];             // [positions 0 / pairs 1]: the slice's counts of the values below HIST_PAIR_LDS_BINS
	const int seg = blockIdx.y, t = threadIdx.x;
	ClassFold f(a);
	if (f.P0 >= f.n) return;                                        // (uniform: the whole workgroup)
	for (int i = t; i < 2 * 4 * HIST_PAIR_LDS_BINS; i += 256) (&bins[0][0][0])[i] = 0;
	f.load(a, rev);
	__syncthreads();                                                // (the mirror is written and the LDS histograms are zero)
	v8u val[4];
#pragma unroll
	for (int c = 0; c < 4; c++) val[c] = f.value(rev, c);           // (zeros for a lane without positions)
	const uint32_t last01 = (uint32_t)val[0][7] | (uint32_t)val[1][7] << 16, last23 = (uint32_t)val[2][7] | (uint32_t)val[3][7] << 16;
	uint32_t prev01 = __shfl_up(last01, 1), prev23 = __shfl_up(last23, 1);
	if ((t & 63) == 63) {
		uint32_t* w = reinterpret_cast<uint32_t*>(&rev[t >> 6][TRACK_CHUNK]);      // (4-byte aligned: a row is 4 096 bytes)
		w[0] = last01; w[1] = last23;
	}
	__syncthreads();
	if ((t & 63) == 0 && t > 0) {
		const uint32_t* w = reinterpret_cast<const uint32_t*>(&rev[(t >> 6) - 1][TRACK_CHUNK]);
		prev01 = w[0]; prev23 = w[1];
	}
	if (f.fwd_on) {
		// (lane 0's predecessor lies in another slice: its prev is never used, p == P0 below)
		uint32_t prev[4] = { prev01 & 0xffffu, prev01 >> 16, prev23 & 0xffffu, prev23 >> 16 };
		const int zh = a.zone[2 * seg], zt = a.zone[2 * seg + 1];
		uint16_t* zbase = a.zones + (int64_t)seg * 8 * a.zstride;
		uint16_t* bbase = a.border + ((int64_t)seg * a.nchunk + blockIdx.x) * 8;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int p = f.p0 + e;
			if (p < f.P1) {
				if (p <= zh && p < a.zstride) {
#pragma unroll
					for (int c = 0; c < 4; c++) zbase[c * a.zstride + p] = val[c][e];
				}
				if (p >= zt - 1 && p - (zt - 1) < a.zstride) {
#pragma unroll
					for (int c = 0; c < 4; c++) zbase[(4 + c) * a.zstride + (p - (zt - 1))] = val[c][e];
				}
				if (p == f.P0) {
#pragma unroll
					for (int c = 0; c < 4; c++) bbase[c] = val[c][e];
				}
				if (p == f.P1 - 1) {
#pragma unroll
					for (int c = 0; c < 4; c++) bbase[4 + c] = val[c][e];
				}
				if (p >= zh && p < zt) {
					const bool pair = p > f.P0 && p - 1 >= zh;
#pragma unroll
					for (int c = 0; c < 4; c++) {
						const uint32_t v = min((uint32_t)val[c][e], (uint32_t)(HIST_BINS - 1));      // (as k_hist)
						if (v < (uint32_t)HIST_PAIR_LDS_BINS) atomicAdd(&bins[0][c][v], 1u);
						else atomicAdd(&a.hist[c * HIST_BINS + v], 1u);
						if (pair) {
							const uint32_t w = min(v, prev[c]);
							if (w < (uint32_t)HIST_PAIR_LDS_BINS) atomicAdd(&bins[1][c][w], 1u);
							else atomicAdd(&a.pairs[c * HIST_BINS + w], 1u);
						}
					}
				}
			}
#pragma unroll
			for (int c = 0; c < 4; c++) prev[c] = (uint32_t)val[c][e];      // (min(v, prev) is clamped through v)
		}
	}
	__syncthreads();
	for (int i = t; i < 2 * 4 * HIST_PAIR_LDS_BINS; i += 256) {
		const uint32_t cnt = (&bins[0][0][0])[i];
		if (!cnt) continue;
		uint32_t* out = i < 4 * HIST_PAIR_LDS_BINS ? a.hist : a.pairs;
		const int k = i % (4 * HIST_PAIR_LDS_BINS);
		atomicAdd(&out[(k / HIST_PAIR_LDS_BINS) * HIST_BINS + (k % HIST_PAIR_LDS_BINS)], cnt);
	}
}

hipError_t launch_hist_pairs(const HistPairsLaunch& L, hipStream_t st)
{
	hipError_t rc;
	if (class_fold_done(L, &rc)) return rc;
	if (L.zstride < 1 || !L.zones || !L.hist || !L.zone || !L.pairs || !L.border) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	hipLaunchKernelGGL(k_hist_pairs, grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
