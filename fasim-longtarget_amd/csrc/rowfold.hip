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

hipError_t launch_rowfold(const RowFoldLaunch& L, hipStream_t st)
{
	if (L.ngroups <= 0) return hipSuccess;
	if (L.rows_total <= 0 || (L.rows_total & 15) != 0 || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	const dim3 grid((unsigned)((L.rows_total / 8 + 255) / 256), (unsigned)L.ngroups);
	hipLaunchKernelGGL(k_rowfold, grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
