// fasim-longtarget_amd/csrc/class_fold.h -- device code shared by the kernels that fold k_scan's maxima by strand class (k_track, k_sites,
// k_hist, k_rowfold): the packed 16-bit vector types, the saturation test, the front half of the three column folds and the lookup of
// the encoding behind a peak.
//
// The front half (ClassFold) turns the column maxima of one slice of TRACK_CHUNK positions into the lane's potential, 8 consecutive
// positions of every class.  One 256-thread workgroup per slice; what it guarantees:
//   * every global load is one aligned 16-byte load inside the row: forward rows at p0 = P0 + 8 t, reversed rows at
//     jg = ((n - P1) & ~7) + 8 t.  P0 and tstride are multiples of 8 and p0 < n <= tstride (jg < n - P0 <= tstride), so the group of
//     8 ends inside the row's tstride columns.  The slice's positions are columns [n - P1, n - P0) of a reversed row, at most 256
//     aligned groups, one per lane;
//   * the masks exclude, before anything is folded or tested for saturation, the forward columns from P1 on (from n on they hold
//     whatever an earlier batch left there) and the reversed columns outside [n - P1, n - P0) (they belong to the neighbouring slices);
//   * load() writes slots [0, P1 - P0) of rev[c][] and no other: slot s is the class maximum of the reversed rows at position P0 + s
//     (column n - 1 - P0 - s).  value() reads slots 8 t .. 8 t + 7 and masks those from P1 - P0 on, which were never written;
//   * slots TRACK_CHUNK .. TRACK_CHUNK + 7 of every row of rev[][] are the caller's: TRACK_CHUNK = 8 x 255, so only lane 255 owns them,
//     it never holds a position (fwd_on is false, value() returns before it reads) and load() writes below P1 - P0 <= TRACK_CHUNK.
//     k_hist_pairs (hist_pairs.hip) keeps its wave-boundary words there; a change to either function must keep this true;
//   * sat[k] = 1 for every unit of the segment with a saturated column maximum among the slice's positions;
//   * all maxima are taken on the raw values (v_pk_max_u16); the taint bit goes with one shift in value(), since
//     max(a, b) >> 1 == max(a >> 1, b >> 1).
// The caller owns rev[][] and the barrier between load() and value(), so that it can prepare LDS arrays of its own ahead of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

typedef unsigned short v8u __attribute__((ext_vector_type(8)));
typedef unsigned short v2us __attribute__((ext_vector_type(2)));
typedef unsigned int v4w __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));

// != 0 when one of the 8 raw values is a saturated column (row) maximum (2 * 16 383 + taint)
__device__ __forceinline__ bool fold_saturated(v8u v)
{
	const v4w w = __builtin_bit_cast(v4w, v);
	const v2us a = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[0]), __builtin_bit_cast(v2us, w[1]));
	const v2us b = __builtin_elementwise_max(__builtin_bit_cast(v2us, w[2]), __builtin_bit_cast(v2us, w[3]));
	const v2us m = __builtin_elementwise_max(a, b);
	return m[0] >= 32766 || m[1] >= 32766;
}

static_assert(TRACK_CHUNK == 8 * 255, "lane 255 owns no position: rev[][TRACK_CHUNK ..] is the caller's (see above)");

struct ClassFold {
	int n, P0, P1;            // the segment's length and the slice's positions [P0, P1); P0 >= n: no such slice, the workgroup returns
	int p0, jlo, jhi, jg;     // the lane's forward columns p0 .. p0 + 7, its reversed columns jg .. jg + 7 of the slice's [jlo, jhi)
	bool fwd_on, rev_on;      // the lane holds a position (a reversed column) of the slice
	const uint16_t* base;     // the segment's rows
	v8u fmask, rmask;
	v8u facc[4];              // class maxima of the forward rows at the lane's positions

	// the geometry of slice blockIdx.x of segment blockIdx.y for lane threadIdx.x (P0 >= n is uniform over the workgroup)
	__device__ __forceinline__ explicit ClassFold(const ClassFoldLaunch& a)
	{
		const int chunk = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
		n = a.seg_len[seg];
		P0 = chunk * TRACK_CHUNK;
		P1 = min(n, P0 + TRACK_CHUNK);
		base = a.colmax16 + (int64_t)seg * a.nenc * a.tstride;
		p0 = P0 + 8 * t;
		fwd_on = p0 < P1;
		jlo = n - P1; jhi = n - P0;
		jg = (jlo & ~7) + 8 * t;
		rev_on = jg < jhi;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			fmask[e] = (p0 + e < P1) ? 0xffff : 0;
			rmask[e] = (jg + e >= jlo && jg + e < jhi) ? 0xffff : 0;
		}
	}

	// the rows of every class through the class table: the forward maxima into facc, the reversed ones mirrored into rev
	__device__ __forceinline__ void load(const ClassFoldLaunch& a, uint16_t (&rev)[4][TRACK_CHUNK + 8])
	{
		uint8_t* sat = a.sat + (int64_t)blockIdx.y * a.nenc;
		v8u racc[4];
#pragma unroll
		for (int c = 0; c < 4; c++) {
			facc[c] = (v8u)(0); racc[c] = (v8u)(0);
			if (fwd_on) {
				for (int i = a.tab.first[c]; i < a.tab.first[c + 1]; i++) {
					const int k = a.tab.k[i];
					const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.tstride + p0) & fmask;
					facc[c] = __builtin_elementwise_max(facc[c], v);
					if (fold_saturated(v)) sat[k] = 1;
				}
			}
			if (rev_on) {
				for (int i = a.tab.first[4 + c]; i < a.tab.first[5 + c]; i++) {
					const int k = a.tab.k[i];
					const v8u v = *reinterpret_cast<const v8u*>(base + (int64_t)k * a.tstride + jg) & rmask;
					racc[c] = __builtin_elementwise_max(racc[c], v);
					if (fold_saturated(v)) sat[k] = 1;
				}
			}
		}
		// column j is position n - 1 - j, slot n - 1 - j - P0 of the slice
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
	}

	// after the barrier: the potential of class c at positions p0 .. p0 + 7 (0 from P1 on)
	__device__ __forceinline__ v8u value(const uint16_t (&rev)[4][TRACK_CHUNK + 8], int c) const
	{
		if (!fwd_on) return (v8u)(0);
		const v8u r = *reinterpret_cast<const v8u*>(&rev[c][8 * threadIdx.x]) & fmask;
		return __builtin_elementwise_max(facc[c], r) >> (v8u)(1);
	}
};

// The smallest index k (0 .. nenc) of an enabled encoding of class c whose unit holds `value` at position pos of the segment, or
// 0x7fffffff: the column again, row by row, forward rows at the position, reversed rows at its mirror image (pos < n <= tstride)
__device__ __forceinline__ int class_peak_encoding(const TrackTable& tab, const uint16_t* base, int tstride, int n, int c, int pos, int value)
{
	int enc = 0x7fffffff;
	for (int i = tab.first[c]; i < tab.first[c + 1]; i++) {
		const int r = tab.k[i];
		if ((int)(base[(int64_t)r * tstride + pos] >> 1) == value) enc = min(enc, r);
	}
	for (int i = tab.first[4 + c]; i < tab.first[5 + c]; i++) {
		const int r = tab.k[i];
		if ((int)(base[(int64_t)r * tstride + (n - 1 - pos)] >> 1) == value) enc = min(enc, r);
	}
	return enc;
}

} // namespace fasim
