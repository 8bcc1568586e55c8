// fasim-longtarget_amd/csrc/track.hip -- k_track: per-base triplex potential tracks for gfx950.
//
// k_scan leaves one number per column of every (segment x encoding) unit: colmax16[unit][column] = 2 * (best local alignment
// score of the lncRNA that ends at that base) + taint bit.  k_track folds the rows of a batch into four tracks per segment, one per
// strand class (ParaPlus, ParaMinus, AntiMinus, AntiPlus): per record bin the maximum over the class's encodings and over the
// positions of the bin.  Column j of an even encoding is position j of the segment, column j of an odd (REV) encoding is position
// n - 1 - j.
//
// A streaming reduction, 2 * nenc * tstride bytes in per segment and at most 4 * 2 * n bytes out, so it is laid out for HBM:
//   * one 256-thread workgroup per slice of TRACK_CHUNK = 2 040 positions of a segment; a lane owns 8 consecutive positions and
//     reads them from every forward row with one aligned 16-byte load (lane after lane: contiguous 4 KB runs per row);
//   * the reversed rows are read the same way, along their COLUMNS: the slice's positions are columns [n - P1, n - P0) there, at most
//     256 aligned groups of 8, one per lane.  The lane keeps their class maxima in registers too and mirrors them through LDS once,
//     after the last row, so no load is ever unaligned or strided;
//   * all maxima are packed 16-bit (v_pk_max_u16 on the raw values: the taint bit is dropped with one shift at the end, since
//     max(a, b) >> 1 == max(a >> 1, b >> 1));
//   * the encodings of a class come from a small table in the kernel arguments (they vary with -r / -t), ordered by class, so the
//     accumulators are never indexed dynamically;
//   * bin == 1: the lane stores its 8 values per class with one 16-byte store.  bin > 1: a lane first joins its own positions into
//     runs of one bin, then the workgroup reduces in LDS (ds_max_u32) and writes each bin of the slice once.  Slices never share an
//     output element (neighbouring slices that touch the same record bin are merged by the host, as overlapping segments are), so
//     there are no global atomics.
//   * peaks (fasim_scan_records_track): the variants with PEAKS also leave, per slice and class, the slice's
//     maximum, its smallest position and the smallest encoding that attains it there.  A lane packs (maximum, 0xffff - first slot of
//     the maximum among its 8 positions) into one word, the word's maximum is taken over the wave with __shfl_xor and over the four
//     waves through LDS, and lane 0 of wave c then reads that one column again from the rows of class c (forward and mirrored, at
//     most 24) for the encoding.  One 16-byte store per (slice, class).  The variant without SLICES (bin == 0) writes nothing else.
//
// The loads, the class maxima, the mirror through LDS and sat[] are the front half that k_sites and k_hist share (class_fold.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "class_fold.h"

namespace fasim {

// SLICES: the binned slices of the tracks go to a.out (bin >= 1); PEAKS: the slice's peak per class goes to a.peaks
template <bool SLICES, bool PEAKS>
__global__ void __launch_bounds__(256) k_track(TrackLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t binacc[4][SLICES ? TRACK_MAX_LDS_BINS : 1];  // bin > 1: the slice's bins
	__shared__ uint32_t wkey[4][PEAKS ? 4 : 1];                     // peaks: per class the four waves' best (value, slot) words
	const int chunk = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
	ClassFold f(a);
	if (f.P0 >= f.n) return;                                        // (uniform: the whole workgroup)
	const int P0 = f.P0, P1 = f.P1, p0 = f.p0;
	f.load(a, rev);
	const int nbc = SLICES && a.bin > 1 ? (int)(((uint32_t)a.phase[seg] + (uint32_t)(P1 - 1)) / (uint32_t)a.bin - ((uint32_t)a.phase[seg] + (uint32_t)P0) / (uint32_t)a.bin) + 1 : 0;
	if constexpr (SLICES) { for (int i = t; i < 4 * nbc; i += 256) binacc[i / nbc][i % nbc] = 0; }
	__syncthreads();
	v8u val[4];
#pragma unroll
	for (int c = 0; c < 4; c++) val[c] = f.value(rev, c);
	if constexpr (PEAKS) {
		// value first, then the smaller slot: the maximum of (value << 16) | (0xffff - slot); lanes past the slice hold zeros
		uint32_t key[4];
#pragma unroll
		for (int c = 0; c < 4; c++) {
			uint32_t best = 0;
#pragma unroll
			for (int e = 0; e < 8; e++) best = max(best, ((uint32_t)val[c][e] << 16) | (uint32_t)(0xffff - (8 * t + e)));
			key[c] = best;
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
			for (int c = 0; c < 4; c++) key[c] = max(key[c], (uint32_t)__shfl_xor((int)key[c], d));
		}
		if ((t & 63) == 0) {
#pragma unroll
			for (int c = 0; c < 4; c++) wkey[c][t >> 6] = key[c];
		}
		__syncthreads();
		if ((t & 63) == 0) {
			const int c = t >> 6;
			const uint32_t k = max(max(wkey[c][0], wkey[c][1]), max(wkey[c][2], wkey[c][3]));
			const int value = (int)(k >> 16);
			v4i pk = { 0, -1, -1, 0 };
			if (value > 0) {
				const int pos = P0 + (int)(0xffff - (k & 0xffff));
				pk = (v4i){ value, pos, class_peak_encoding(a.tab, f.base, a.tstride, f.n, c, pos, value), 0 };
			}
			*reinterpret_cast<v4i*>(a.peaks + ((int64_t)seg * a.nchunk + chunk) * 4 + c) = pk;
		}
	}
	if constexpr (!SLICES) return;
	const int stride = track_slice_stride(a.bin);
	uint16_t* out = a.out + ((int64_t)seg * a.nchunk + chunk) * 4 * stride;
	if (a.bin == 1) {
		// one value per position: slot 8 t .. 8 t + 7 of the slice (8 * 254 + 7 < stride = 2 040; positions from P1 on store 0)
		if (f.fwd_on) {
#pragma unroll
			for (int c = 0; c < 4; c++) *reinterpret_cast<v8u*>(out + c * stride + 8 * t) = val[c];
		}
		return;
	}
	if (f.fwd_on) {
		// the lane's positions as runs of one bin each; a run's maximum goes to the slice's bin in LDS (zeros need not)
		const uint32_t x0 = (uint32_t)a.phase[seg] + (uint32_t)p0, bin = (uint32_t)a.bin;
		uint32_t b = x0 / bin - ((uint32_t)a.phase[seg] + (uint32_t)P0) / bin;      // bin within the slice
		uint32_t r = x0 % bin;
		uint32_t run[4] = { 0, 0, 0, 0 };
#pragma unroll
		for (int e = 0; e < 8; e++) {
#pragma unroll
			for (int c = 0; c < 4; c++) run[c] = max(run[c], (uint32_t)val[c][e]);
			if (++r == bin || e == 7) {
#pragma unroll
				for (int c = 0; c < 4; c++) { if (run[c] && b < (uint32_t)nbc) atomicMax(&binacc[c][b], run[c]); run[c] = 0; }
				b++; r = 0;
			}
		}
	}
	__syncthreads();
	for (int i = t; i < 4 * nbc; i += 256) { const int c = i / nbc, k = i % nbc; out[c * stride + k] = (uint16_t)binacc[c][k]; }
}

hipError_t launch_track(const TrackLaunch& L, hipStream_t st)
{
	hipError_t rc;
	if (class_fold_done(L, &rc)) return rc;
	if (L.bin < 0 || (L.bin == 0 && !L.peaks)) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	if (!L.peaks) hipLaunchKernelGGL((k_track<true, false>), grid, dim3(256), 0, st, L);
	else if (L.bin >= 1) hipLaunchKernelGGL((k_track<true, true>), grid, dim3(256), 0, st, L);
	else hipLaunchKernelGGL((k_track<false, true>), grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
