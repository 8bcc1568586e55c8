// fasim-longtarget_amd/csrc/hist.hip -- k_hist: histogram of the per-base triplex potential over the positions of a batch, for gfx950.
//
// The potential of a segment is what k_track (track.hip) folds from k_scan's column maxima: per strand class the maximum over the
// class's encodings, forward rows by column, reversed rows mirrored.  k_hist folds the same values and, instead of storing them,
// counts them: hist[class][value] += 1 for every position of the batch.  A call then copies back 4 x 16 384
// counters per batch, and less for a short query, instead of 4 x 2 bytes per base.
//
//   * the front half is the one k_track uses (class_fold.h): one 256-thread workgroup per slice of TRACK_CHUNK = 2 040 positions,
//     a lane owns 8 consecutive positions;
//   * a position that a neighbouring segment of the record covers too (the segment's head or tail zone, bounds from the host) is
//     not counted here: a base counts once, with the maximum of its two segments, and only the host sees both.  Its four values go
//     to the batch's zone buffer, 2 x overlapLength positions per segment at most;
//   * every other position is counted into a workgroup histogram in LDS, 4 classes x HIST_LDS_BINS counters (ds_add_u32), which is
//     flushed after a barrier: one global atomic add per non-zero bin.  A value of HIST_LDS_BINS or more is rare (a potential of
//     1 024 is an alignment of more than 200 matches) and goes to HBM at once;
//   * sums of integers do not depend on their order: the result is the same bit for bit on every run, whatever the schedule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "class_fold.h"

namespace fasim {

__global__ void __launch_bounds__(256) k_hist(HistLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t bins[4][HIST_LDS_BINS];                     // the slice's counts of the values below HIST_LDS_BINS
	const int seg = blockIdx.y, t = threadIdx.x;
	ClassFold f(a);
	if (f.P0 >= f.n) return;                                        // (uniform: the whole workgroup)
	for (int i = t; i < 4 * HIST_LDS_BINS; i += 256) (&bins[0][0])[i] = 0;
	f.load(a, rev);
	__syncthreads();                                                // (the mirror is written and the LDS histogram is zero)
	if (f.fwd_on) {
		v8u val[4];
#pragma unroll
		for (int c = 0; c < 4; c++) val[c] = f.value(rev, c);
		const int zh = a.zone[2 * seg], zt = a.zone[2 * seg + 1];
		uint16_t* zbase = a.zones + (int64_t)seg * 8 * a.zstride;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int p = f.p0 + e;
			if (p >= f.P1) continue;
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
	hipError_t rc;
	if (class_fold_done(L, &rc)) return rc;
	if (L.zstride < 0 || (L.zstride > 0 && !L.zones) || !L.hist || !L.zone) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	hipLaunchKernelGGL(k_hist, grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
