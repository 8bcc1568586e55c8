// fasim-longtarget_amd/csrc/rowfold.hip -- k_rowfold: the per-base profile of the lncRNA for gfx950.
//
// The ROWS variant of k_scan leaves one number per query row of every (segment x encoding) unit: rowmax16[unit][row] = 2 * (best
// local alignment score that ends on that base of the lncRNA, over the unit's real columns) + taint bit.  k_rowfold folds the units
// of a group of segments (the segments of one record, or the whole batch) into four profiles, one per strand class (ParaPlus,
// ParaMinus, AntiMinus, AntiPlus).  The query is never reversed, so row i is base i of the lncRNA for every encoding and the
// reversed encodings need no mirroring: they are just more rows of their class.
//
// A streaming reduction like k_track, 2 * nenc * rows_total bytes in per segment and 4 * 2 * rows_total bytes out per group:
//   * one 256-thread workgroup per slice of 2 048 rows of a group; a lane owns 8 consecutive rows and reads them from every unit of
//     the group with one aligned 16-byte load (rows_total is a multiple of 16, so every load is aligned and in range);
//   * packed 16-bit maxima (v_pk_max_u16) on the raw values; the taint bit is dropped with one shift at the end
//     (max(a, b) >> 1 == max(a >> 1, b >> 1));
//   * the encodings of a class come from the table k_track uses, ordered by class, so the accumulators are never indexed dynamically;
//   * one 16-byte store per (group, class, lane): every output element has one writer, no global atomics.
// k_rowfold_parts, below it, gives the same result for an oligo of a panel from the parts of k_scan_short_rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "class_fold.h"

namespace fasim {

__global__ void __launch_bounds__(256) k_rowfold(RowFoldLaunch a)
{
	const int g = blockIdx.y;
	const int r0 = (blockIdx.x * 256 + threadIdx.x) * 8;          // my rows r0 .. r0 + 7 (rows_total is a multiple of 8)
	if (r0 >= a.rows_total) return;
	const int s0 = a.gfirst[g], s1 = a.gfirst[g + 1];
	v8u acc[4];
#pragma unroll
	for (int c = 0; c < 4; c++) acc[c] = (v8u)(0);
	for (int s = s0; s < s1; s++) {
		const uint16_t* base = a.rowmax16 + (int64_t)s * a.nenc * a.rows_total + r0;
		uint8_t* sat = a.sat + (int64_t)s * a.nenc;
#pragma unroll
		for (int c = 0; c < 4; c++) {
			// forward and reversed encodings of class c
			for (int half = 0; half < 2; half++) {
				for (int i = a.tab.first[4 * half + c]; i < a.tab.first[4 * half + c + 1]; i++) {
					const int k = a.tab.k[i];
					const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.rows_total);
					acc[c] = __builtin_elementwise_max(acc[c], v);
					if (fold_saturated(v)) sat[k] = 1;
				}
			}
		}
	}
	uint16_t* out = a.out + (int64_t)g * 4 * a.rows_total + r0;
#pragma unroll
	for (int c = 0; c < 4; c++) *reinterpret_cast<v8u*>(out + (int64_t)c * a.rows_total) = acc[c] >> (v8u)(1);
}

// ---- k_rowfold_parts: the profile of an oligo from the parts of k_scan_short_rows -----------------------------
// An oligo has at most 112 rows, 14 chunks of 8, and a group has tens of thousands of parts (units x stretch pairs): the parallel
// axis is the parts.  One 256-thread workgroup per (group, class); lane t owns row chunk t % nchunk of the parts slice, slice + nslice,
// ... of the class, slice = t / nchunk, so the lanes of neighbouring chunks read one part's neighbouring 16 bytes.  The parts of a
// class are (segment of the group) x (encoding of the class, forward and reversed alike: the query is never mirrored) x (pair); a
// part whose lane returned before it wrote (2 * pair * stretch >= unit_len) is skipped.  v_pk_max_u16 on the raw values, an LDS tree
// over the slices, the taint bit dropped with one shift, one 16-byte store per (group, class, row chunk): one writer per element.
__global__ void __launch_bounds__(256) k_rowfold_parts(RowPartFoldLaunch a)
{
	__shared__ v8u red[256];
	const int g = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
	const int nchunk = a.rows / 8, nslice = 256 / nchunk;
	const int slice = t / nchunk, chunk = t - slice * nchunk;
	const int s0 = a.gfirst[g], s1 = a.gfirst[g + 1];
	const int f0 = a.tab.first[c], nf = a.tab.first[c + 1] - f0, r0 = a.tab.first[4 + c], nk = nf + a.tab.first[5 + c] - r0;
	v8u acc = (v8u)(0);
	if (slice < nslice) {
		const int nparts = (s1 - s0) * nk * a.npairs;
		for (int p = slice; p < nparts; p += nslice) {
			const int x = p / a.npairs, pair = p - x * a.npairs, s = x / nk, kk = x - s * nk;
			const int unit = (s0 + s) * a.nenc + a.tab.k[kk < nf ? f0 + kk : r0 + kk - nf];
			if (2 * pair * a.stretch >= a.unit_len[unit]) continue;
			const v8u v = *reinterpret_cast<const v8u*>(a.rowpart16 + ((int64_t)unit * a.npairs + pair) * a.rows + 8 * chunk);
			acc = __builtin_elementwise_max(acc, v);
		}
	}
	red[t] = acc;
	__syncthreads();
	// slices [h, nslice) onto [0, nslice - h): nslice <= 2 h at the first h that does anything
	for (int h = 128; h >= 1; h >>= 1) {
		if (slice < h && slice + h < nslice) red[t] = __builtin_elementwise_max(red[t], red[t + h * nchunk]);
		__syncthreads();
	}
	if (slice == 0) *reinterpret_cast<v8u*>(a.out + ((int64_t)g * 4 + c) * a.rows + 8 * chunk) = red[t] >> (v8u)(1);
}

hipError_t launch_rowfold_parts(const RowPartFoldLaunch& L, hipStream_t st)
{
	if (L.ngroups <= 0) return hipSuccess;
	if (L.rows < 16 || L.rows > 112 || (L.rows & 15) != 0 || L.nenc < 1 || L.nenc > 48 || L.npairs < 1 || L.stretch < 16) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_rowfold_parts, dim3((unsigned)L.ngroups, 4), dim3(256), 0, st, L);
	return hipGetLastError();
}

hipError_t launch_rowfold(const RowFoldLaunch& L, hipStream_t st)
{
	if (L.ngroups <= 0) return hipSuccess;
	if (L.rows_total <= 0 || (L.rows_total & 15) != 0 || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	const dim3 grid((unsigned)((L.rows_total / 8 + 255) / 256), (unsigned)L.ngroups);
	hipLaunchKernelGGL(k_rowfold, grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
