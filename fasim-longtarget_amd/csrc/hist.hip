// fasim-longtarget_amd/csrc/hist.hip -- k_hist: histogram of the per-base triplex potential over the positions of a batch, for gfx950.
//
// The potential of a segment is what k_track (track.hip) folds from k_scan's column maxima: per strand class the maximum over the
// class's encodings, forward rows by column, reversed rows mirrored.  k_hist folds the same values and, instead of storing them,
// counts them: hist[class][value] += 1 for every position of the batch.  A call then copies back 4 x 16 384
// counters per batch, and less for a short query, instead of 4 x 2 bytes per base.
//
//   * the front half is k_track's: one 256-thread workgroup per slice of TRACK_CHUNK = 2 040 positions, a lane owns 8 consecutive
//     positions, aligned 16-byte loads of the forward rows, the reversed rows read along their columns and mirrored once through
//     LDS, v_pk_max_u16 on the raw values through the class table in the kernel arguments, the taint bit shifted out at the end,
//     sat[unit] set.  It is the third copy (track.hip, sites.hip), kept apart so that the instantiations there compile as before:
//     a change to the loads or to the class table belongs in all three files;
//   * a position that a neighbouring segment of the record covers too (the segment's head or tail zone, bounds from the host) is
//     not counted here: a base counts once, with the maximum of its two segments, and only the host sees both.  Its four values go
//     to the batch's zone buffer, 2 x overlapLength positions per segment at most;
//   * every other position is counted into a workgroup histogram in LDS, 4 classes x HIST_LDS_BINS counters (ds_add_u32), which is
//     flushed after a barrier: one global atomic add per non-zero bin.  A value of HIST_LDS_BINS or more is rare (a potential of
//     1 024 is an alignment of more than 200 matches) and goes to HBM at once;
//   * sums of integers do not depend on their order: the result is the same bit for bit on every run, whatever the schedule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

typedef unsigned short v8u __attribute__((ext_vector_type(8)));
typedef unsigned short v2us __attribute__((ext_vector_type(2)));
typedef unsigned int v4w __attribute__((ext_vector_type(4)));

// != 0 when one of the 8 raw values is a saturated column maximum (2 * 16 383 + taint)
__device__ __forceinline__ bool hist_saturated(v8u v)
{
	const v4w w = __builtin_bit_cast(v4w, v);
	const v2us a = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[0]), __builtin_bit_cast(v2us, w[1]));
	const v2us b = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[2]), __builtin_bit_cast(v2us, w[3]));
	const v2us m = __builtin_elementwise_max(a, b);
	return m[0] >= 32766 || m[1] >= 32766;
}

__global__ void __launch_bounds__(256) k_hist(HistLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t bins[4][HIST_LDS_BINS];                     // the slice's counts of the values below HIST_LDS_BINS
	const int chunk = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
	const int n = a.seg_len[seg];
	const int P0 = chunk * TRACK_CHUNK;
	if (P0 >= n) return;                                            // (uniform: the whole workgroup)
	const int P1 = min(n, P0 + TRACK_CHUNK);
	const uint16_t* base = a.colmax16 + (int64_t)seg * a.nenc * a.tstride;
	uint8_t* sat = a.sat + (int64_t)seg * a.nenc;
	for (int i = t; i < 4 * HIST_LDS_BINS; i += 256) (&bins[0][0])[i] = 0;

	// forward rows: positions p0 .. p0 + 7 (p0 + 7 < tstride: P0 and tstride are multiples of 8 and p0 < n <= tstride)
	const int p0 = P0 + 8 * t;
	const bool fwd_on = p0 < P1;
	// reversed rows: columns jg .. jg + 7 of the aligned groups that cover [n - P1, n - P0) (jg + 7 < tstride as above)
	const int jlo = n - P1, jhi = n - P0;
	const int jg = (jlo & ~7) + 8 * t;
	const bool rev_on = jg < jhi;
	// columns from n on hold whatever an earlier batch left there; reversed columns outside the slice belong to its neighbours
	v8u fmask, rmask;
#pragma unroll
	for (int e = 0; e < 8; e++) {
		fmask[e] = (p0 + e < P1) ? 0xffff : 0;
		rmask[e] = (jg + e >= jlo && jg + e < jhi) ? 0xffff : 0;
	}
	v8u facc[4], racc[4];
#pragma unroll
	for (int c = 0; c < 4; c++) {
		facc[c] = (v8u)(0); racc[c] = (v8u)(0);
		if (fwd_on) {
			for (int i = a.tab.first[c]; i < a.tab.first[c + 1]; i++) {
				const int k = a.tab.k[i];
				const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.tstride + p0) & fmask;
				facc[c] = __builtin_elementwise_max(facc[c], v);
				if (hist_saturated(v)) sat[k] = 1;
			}
		}
		if (rev_on) {
			for (int i = a.tab.first[4 + c]; i < a.tab.first[5 + c]; i++) {
				const int k = a.tab.k[i];
				const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.tstride + jg) & rmask;
				racc[c] = __builtin_elementwise_max(racc[c], v);
				if (hist_saturated(v)) sat[k] = 1;
			}
		}
	}
	// mirror the reversed maxima: column j is position n - 1 - j, slot n - 1 - j - P0 of the slice (every slot of [0, P1 - P0) is
	// written: its column lies in [jlo, jhi))
	if (rev_on) {
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int j = jg + e;
			if (j >= jlo && j < jhi) {
				const int slot = n - 1 - j - P0;
#pragma unroll
				for (int c = 0; c < 4; c++) rev[c][slot] = racc[c][e];
			}
		}
	}
	__syncthreads();                                                // (the mirror is written and the LDS histogram is zero)
	if (fwd_on) {
		v8u val[4];
#pragma unroll
		for (int c = 0; c < 4; c++) {
			const v8u r = *reinterpret_cast<const v8u*>(&rev[c][8 * t]) & fmask;      // (slots from P1 - P0 on were never written)
			val[c] = __builtin_elementwise_max(facc[c], r) >> (v8u)(1);
		}
		const int zh = a.zone[2 * seg], zt = a.zone[2 * seg + 1];
		uint16_t* zbase = a.zones + (int64_t)seg * 8 * a.zstride;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int p = p0 + e;
			if (p >= P1) continue;
			if (p < zh || p >= zt) {
				// head zone: slot p of zones[seg][0]; tail zone: slot p - zt of zones[seg][1]
				const int slot = p < zh ? p : p - zt;
				if (slot < a.zstride) {
					uint16_t* z = zbase + (p < zh ? 0 : 4 * a.zstride) + slot;
#pragma unroll
					for (int c = 0; c < 4; c++) z[c * a.zstride] = val[c][e];
				}
				continue;
			}
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const uint32_t v = min((uint32_t)val[c][e], (uint32_t)(HIST_BINS - 1));
				if (v < (uint32_t)HIST_LDS_BINS) atomicAdd(&bins[c][v], 1u);
				else atomicAdd(&a.hist[c * HIST_BINS + v], 1u);
			}
		}
	}
	__syncthreads();
	for (int i = t; i < 4 * HIST_LDS_BINS; i += 256) {
		const uint32_t cnt = (&bins[0][0])[i];
		if (cnt) atomicAdd(&a.hist[(i / HIST_LDS_BINS) * HIST_BINS + (i % HIST_LDS_BINS)], cnt);
	}
}

hipError_t launch_hist(const HistLaunch& L, hipStream_t st)
{
	if (L.nseg <= 0 || L.nchunk <= 0) return hipSuccess;
	if ((L.tstride & 7) != 0 || L.nenc < 1 || L.nenc > 48 || L.zstride < 0 || (L.zstride > 0 && !L.zones) || !L.hist || !L.zone) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	hipLaunchKernelGGL(k_hist, grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
