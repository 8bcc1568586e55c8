// fasim-longtarget_amd/csrc/sites.hip -- k_sites: the runs of positions whose triplex potential reaches a fixed value, for gfx950.
//
// The potential of a segment is what k_track (track.hip) folds from k_scan's column maxima: per strand class the maximum over
// the class's encodings, forward rows by column, reversed rows mirrored.  k_sites folds the same values and, instead of storing
// them, leaves the RUNS of every class: maximal ranges of positions of one slice whose potential is >= min_value, each with its
// largest value, the smallest position that attains it and the smallest encoding that attains it there.
// The slice edge cuts runs; the host joins them again by their coordinates, as it joins the runs of overlapping segments.
//
//   * the front half is the one k_track uses (class_fold.h): one 256-thread workgroup per slice of TRACK_CHUNK = 2 040 positions,
//     a lane owns 8 consecutive positions;
//   * a lane walks its own 8 slots only.  What a run needs from the lanes before it -- whether it is still open at the lane's
//     first slot, where it started and the best (value << 16) | (0xffff - slot) word so far -- is a carry (open, start, key), and
//     the carries are combined by a segmented max-scan: __shfl_up over the wave (6 steps), then the four waves' totals through
//     LDS.  A lane whose 8 slots are all flagged hands the carry on (extended by its own key), every other lane starts a new one.
//     So the pass streams whatever the run structure is: 1 020 runs per class and slice cost what none costs, apart from the
//     stores;
//   * the lane that owns a run's last slot emits it (the first flag of the next lane's slots comes through LDS), at most 4 per
//     class and lane.  The runs' places in the output follow from an add-scan of the lanes' run counts, so the output is in
//     position order and the same on every run;
//   * two launches of one template, no capacity guess: COUNT writes the run count per (slice, class), the host takes the prefix
//     sum and sizes the buffer, EMIT writes 16-byte records at those offsets with one vector store each.  The emitting lane reads
//     the run's peak column again from the rows of the class (forward at pos, reversed at n - 1 - pos, at most 24 two-byte loads)
//     for the encoding, as k_track's peak variant does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "class_fold.h"

namespace fasim {

// The carry of the segmented scan, for a range of slots: `key` = the best word of the flagged stretch that ends on the range's last
// slot, `info` = its first slot | OPEN (the last slot is flagged) | FULL (every slot of the range is flagged; the empty range is FULL
// and not OPEN).
constexpr uint32_t SITES_OPEN = 1u << 16, SITES_FULL = 1u << 17;
struct SitesCarry { uint32_t key, info; };
// the carry of range L followed by range R
__device__ __forceinline__ SitesCarry sites_join(SitesCarry l, SitesCarry r)
{
	const bool ext = (r.info & SITES_FULL) && (l.info & SITES_OPEN);      // R's stretch is all of R and goes on into L's
	SitesCarry o;
	o.key = ext ? max(l.key, r.key) : r.key;
	const uint32_t full = (l.info & r.info) & SITES_FULL;
	o.info = ext ? ((l.info & ~SITES_FULL) | full) : ((r.info & ~SITES_FULL) | full);
	return o;
}

// EMIT false: a.counts[slice * 4 + class] = runs of the slice; EMIT true: the runs themselves at a.offsets[slice * 4 + class]
template <bool EMIT>
__global__ void __launch_bounds__(256) k_sites(SitesLaunch a)
{
	__shared__ __align__(16) uint16_t rev[4][TRACK_CHUNK + 8];      // class maxima of the reversed rows, by position within the slice
	__shared__ uint32_t wcarry[4][4][2];                            // per class the four waves' carries
	__shared__ uint32_t wcount[4][2];                               // the four waves' run counts, classes 0|1 and 2|3 packed
	__shared__ uint8_t first_flag[256 + 4];                         // per lane: bit c = the lane's first slot is flagged in class c
	const int chunk = blockIdx.x, seg = blockIdx.y, t = threadIdx.x;
	ClassFold f(a);
	if (f.P0 >= f.n) return;                                        // (uniform: the whole workgroup; the caller zeroed the counts)
	const int P0 = f.P0;
	f.load(a, rev);
	__syncthreads();
	v8u val[4];
#pragma unroll
	for (int c = 0; c < 4; c++) val[c] = f.value(rev, c);

	// ---- the lane's own slots: flags (bit e = slot 8 t + e reaches min_value; slots past the slice hold 0 < min_value), the
	//      carry of its 8 slots and the number of runs that end in them
	const int lane = t & 63, wave = t >> 6;
	const uint32_t vmin = (uint32_t)a.min_value;
	uint32_t flags[4];
	SitesCarry own[4];
	uint32_t ff = 0;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		uint32_t f = 0, key = 0, start = 0;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const uint32_t v = val[c][e];
			const bool on = v >= vmin;
			f |= on ? (1u << e) : 0u;
			const uint32_t k = (v << 16) | (uint32_t)(0xffff - (8 * t + e));
			if (on) { if (e == 0 || !((f >> (e - 1)) & 1)) { start = (uint32_t)(8 * t + e); key = 0; } key = max(key, k); }
		}
		flags[c] = f;
		own[c].key = (f >> 7) & 1 ? key : 0;
		own[c].info = start | ((f >> 7) & 1 ? SITES_OPEN : 0) | (f == 0xff ? SITES_FULL : 0);
		ff |= (f & 1) << c;
	}
	first_flag[t] = (uint8_t)ff;
	if (t < 4) first_flag[256 + t] = 0;                              // (lane 255 owns no slot of the slice: nothing follows slot 2 039)

	// ---- segmented max-scan of the carries over the wave (inclusive), then the carry INTO the lane: that of the lane before it
	SitesCarry inc[4];
#pragma unroll
	for (int c = 0; c < 4; c++) inc[c] = own[c];
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
		for (int c = 0; c < 4; c++) {
			SitesCarry l;
			l.key = (uint32_t)__shfl_up((int)inc[c].key, d);
			l.info = (uint32_t)__shfl_up((int)inc[c].info, d);
			if (lane >= d) inc[c] = sites_join(l, inc[c]);
		}
	}
	if (lane == 63) {
#pragma unroll
		for (int c = 0; c < 4; c++) { wcarry[c][wave][0] = inc[c].key; wcarry[c][wave][1] = inc[c].info; }
	}
	SitesCarry in[4];
#pragma unroll
	for (int c = 0; c < 4; c++) {
		in[c].key = (uint32_t)__shfl_up((int)inc[c].key, 1);
		in[c].info = (uint32_t)__shfl_up((int)inc[c].info, 1);
		if (lane == 0) { in[c].key = 0; in[c].info = SITES_FULL; }      // the empty range
	}
	__syncthreads();
#pragma unroll
	for (int c = 0; c < 4; c++) {
		SitesCarry pre = { 0, SITES_FULL };
		for (int w = 0; w < wave; w++) { const SitesCarry x = { wcarry[c][w][0], wcarry[c][w][1] }; pre = sites_join(pre, x); }
		in[c] = sites_join(pre, in[c]);
	}
	// runs that end in the lane's slots: a flagged slot whose successor is not (slot 7: the next lane's first slot)
	const uint32_t nf = first_flag[t + 1];
	uint32_t ends[4];
	uint32_t cnt01 = 0, cnt23 = 0;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const uint32_t next = (flags[c] >> 1) | (((nf >> c) & 1) << 7);
		ends[c] = flags[c] & ~next;
		const uint32_t k = (uint32_t)__builtin_popcount(ends[c]);
		if (c < 2) cnt01 += k << (16 * c); else cnt23 += k << (16 * (c - 2));
	}
	// add-scan of the run counts (at most 1 020 per class and slice: 16 bits each)
	uint32_t s01 = cnt01, s23 = cnt23;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t x = (uint32_t)__shfl_up((int)s01, d), y = (uint32_t)__shfl_up((int)s23, d);
		if (lane >= d) { s01 += x; s23 += y; }
	}
	if (lane == 63) { wcount[wave][0] = s01; wcount[wave][1] = s23; }
	__syncthreads();
	if constexpr (!EMIT) {
		if (t < 4) {
			const uint32_t w = t < 2 ? wcount[0][0] + wcount[1][0] + wcount[2][0] + wcount[3][0] : wcount[0][1] + wcount[1][1] + wcount[2][1] + wcount[3][1];
			a.counts[((int64_t)seg * a.nchunk + chunk) * 4 + t] = (w >> (16 * (t & 1))) & 0xffff;
		}
		return;
	} else {
		uint32_t b01 = s01 - cnt01, b23 = s23 - cnt23;                 // exclusive: runs of the slice that end before this lane
		for (int w = 0; w < wave; w++) { b01 += wcount[w][0]; b23 += wcount[w][1]; }
#pragma unroll
		for (int c = 0; c < 4; c++) {
			if (!ends[c]) continue;
			uint32_t at = a.offsets[((int64_t)seg * a.nchunk + chunk) * 4 + c] + (((c < 2 ? b01 : b23) >> (16 * (c & 1))) & 0xffff);
			bool open = (in[c].info & SITES_OPEN) != 0;
			uint32_t start = in[c].info & 0xffff, key = in[c].key;
#pragma unroll
			for (int e = 0; e < 8; e++) {
				if (!((flags[c] >> e) & 1)) { open = false; continue; }
				if (!open) { open = true; start = (uint32_t)(8 * t + e); key = 0; }
				key = max(key, ((uint32_t)val[c][e] << 16) | (uint32_t)(0xffff - (8 * t + e)));
				if (!((ends[c] >> e) & 1)) continue;
				// the run [start, 8 t + e] of the slice
				const int value = (int)(key >> 16);
				const int pos = P0 + (int)(0xffff - (key & 0xffff));
				const int enc = class_peak_encoding(a.tab, f.base, a.tstride, f.n, c, pos, value);
				const v4i rec = { P0 + (int)start, P0 + 8 * t + e + 1, value | (enc << 16), pos };
				*reinterpret_cast<v4i*>(a.runs + at) = rec;
				at++;
			}
		}
	}
}

hipError_t launch_sites(const SitesLaunch& L, bool emit, hipStream_t st)
{
	hipError_t rc;
	if (class_fold_done(L, &rc)) return rc;
	if (L.min_value < 1 || L.min_value > 16383) return hipErrorInvalidValue;
	if (emit ? (!L.offsets || !L.runs) : !L.counts) return hipErrorInvalidValue;
	const dim3 grid((unsigned)L.nchunk, (unsigned)L.nseg);
	if (emit) hipLaunchKernelGGL((k_sites<true>), grid, dim3(256), 0, st, L);
	else hipLaunchKernelGGL((k_sites<false>), grid, dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
