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
// k_sites (sites.hip) carries a copy of this kernel's front half (the loads, the class maxima, the mirror through LDS, sat[]), kept
// apart so that the instantiations here compile as before: a change to the loads or to the class table belongs in both files.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

typedef unsigned short v8u __attribute__((ext_vector_type(8)));
typedef unsigned short v2us __attribute__((ext_vector_type(2)));
typedef unsigned int v4w __attribute__((ext_vector_type(4)));

// != 0 when one of the 8 raw values is a saturated column maximum (2 * 16 383 + taint)
__device__ __forceinline__ bool track_saturated(v8u v)
{
	const v4w w = __builtin_bit_cast(v4w, v);
	const v2us a = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[0]), __builtin_bit_cast(v2us, w[1]));
	const v2us b = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[2]), __builtin_bit_cast(v2us, w[3]));
	const v2us m = __builtin_elementwise_max(a, b);
	return m[0] >= 32766 || m[1] >= 32766;
}

typedef int v4i __attribute__((ext_vector_type(4)));

// SLICES: the binned slices of the tracks go to a.out (bin >= 1); PEAKS: the slice's peak per class goes to a.peaks
template <bool SLICES, bool PEAKS>
__global__ void __launch_bounds__(256) k_track(TrackLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t binacc[4][SLICES ? TRACK_MAX_LDS_BINS : 1];  // bin > 1: the slice's bins
	__shared__ uint32_t wkey[4][PEAKS ? 4 : 1];                     // peaks: per class the four waves' best (value, slot) words
	const int chunk = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
	const int n = a.seg_len[seg];
	const int P0 = chunk * TRACK_CHUNK;
	if (P0 >= n) return;                                            // (uniform: the whole workgroup)
	const int P1 = min(n, P0 + TRACK_CHUNK);
	const uint16_t* base = a.colmax16 + (int64_t)seg * a.nenc * a.tstride;
	uint8_t* sat = a.sat + (int64_t)seg * a.nenc;

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
				if (track_saturated(v)) sat[k] = 1;
			}
		}
		if (rev_on) {
			for (int i = a.tab.first[4 + c]; i < a.tab.first[5 + c]; i++) {
				const int k = a.tab.k[i];
				const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.tstride + jg) & rmask;
				racc[c] = __builtin_elementwise_max(racc[c], v);
				if (track_saturated(v)) sat[k] = 1;
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
	const int nbc = SLICES && a.bin > 1 ? (int)(((uint32_t)a.phase[seg] + (uint32_t)(P1 - 1)) / (uint32_t)a.bin - ((uint32_t)a.phase[seg] + (uint32_t)P0) / (uint32_t)a.bin) + 1 : 0;
	if constexpr (SLICES) { for (int i = t; i < 4 * nbc; i += 256) binacc[i / nbc][i % nbc] = 0; }
	__syncthreads();
	v8u val[4];
#pragma unroll
	for (int c = 0; c < 4; c++) {
		val[c] = (v8u)(0);
		if (fwd_on) {
			const v8u r = *reinterpret_cast<const v8u*>(&rev[c][8 * t]) & fmask;      // (slots from P1 - P0 on were never written)
			val[c] = __builtin_elementwise_max(facc[c], r) >> (v8u)(1);
		}
	}
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
				// the column again, row by row: forward rows at the position, reversed rows at its mirror image (pos < P1 <= n <= tstride)
				const int pos = P0 + (int)(0xffff - (k & 0xffff));
				int enc = 0x7fffffff;
				for (int i = a.tab.first[c]; i < a.tab.first[c + 1]; i++) {
					const int r = a.tab.k[i];
					if ((int)(base[(int64_t)r * a.tstride + pos] >> 1) == value) enc = min(enc, r);
				}
				for (int i = a.tab.first[4 + c]; i < a.tab.first[5 + c]; i++) {
					const int r = a.tab.k[i];
					if ((int)(base[(int64_t)r * a.tstride + (n - 1 - pos)] >> 1) == value) enc = min(enc, r);
				}
				pk = (v4i){ value, pos, enc, 0 };
			}
			*reinterpret_cast<v4i*>(a.peaks + ((int64_t)seg * a.nchunk + chunk) * 4 + c) = pk;
		}
	}
	if constexpr (!SLICES) return;
	const int stride = track_slice_stride(a.bin);
	uint16_t* out = a.out + ((int64_t)seg * a.nchunk + chunk) * 4 * stride;
	if (a.bin == 1) {
		// one value per position: slot 8 t .. 8 t + 7 of the slice (8 * 254 + 7 < stride = 2 040; positions from P1 on store 0)
		if (fwd_on) {
#pragma unroll
			for (int c = 0; c < 4; c++) *reinterpret_cast<v8u*>(out + c * stride + 8 * t) = val[c];
		}
		return;
	}
	if (fwd_on) {
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
	if (L.nseg <= 0 || L.nchunk <= 0) return hipSuccess;
	if (L.bin < 0 || (L.bin == 0 && !L.peaks) || (L.tstride & 7) != 0 || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	if (!L.peaks) hipLaunchKernelGGL((k_track<true, false>), grid, dim3(256), 0, st, L);
	else if (L.bin >= 1) hipLaunchKernelGGL((k_track<true, true>), grid, dim3(256), 0, st, L);
	else hipLaunchKernelGGL((k_track<false, true>), grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
