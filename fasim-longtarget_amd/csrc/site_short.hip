// fasim-longtarget_amd/csrc/site_short.hip -- k_site_ends_short: end and start cell of the hit of an oligo's site, one problem per
// lane, for gfx950.
//
// The hit of a site is section 15's (site_align.hip): pass (i) finds the end cell (i1, j1) in the local matrix H, pass (ii) the
// start cell (i0, j0) in the matrix anchored at the end cell, pass (iii) the path.  k_site_ends gives a problem a workgroup and
// sweeps the prefix [0, jp] of the unit.  For an oligo of m <= 112 nt both are waste: no positive-scoring alignment spans more
// than W(m) = ROWS + max(0, (5 m - 13) div 4) columns (section 16), so the columns [jp - 15, jp] that decide the end cell are
// exact in a matrix started from zeros at column jp - 15 - W(m), and the whole DP column (ROWS = 16 * ceil(m / 16) rows of H and
// E) fits a lane's registers, as in k_scan_short.
//
//   * one problem per lane, 256 consecutive problems per workgroup; the arithmetic is 32-bit, so "no path" is a plain -2^20
//     that neither wraps nor climbs back to a value >= 1 within the at most 266 + 250 columns of a problem;
//   * the oligo is uniform over the launch: prof[row][target code] (the forward pass: one ds_read whose row offset is an
//     immediate) and the codes themselves behind ROWS guard entries of code N (the reverse pass: row r of the anchored matrix is
//     query row i1 - r, indexed per lane; the rows past query row 0 read the guard, feed nothing back and are never a start);
//   * pass (i): columns [(jp & ~15) - warm, (jp | 15)], warm = W(m) + 16: warm / 16 + 1 groups of 16 columns for every lane of
//     the launch, each one aligned 16-byte load from the problem's own unit (the host pads a unit's row to a multiple of 16 with
//     code N); columns before the unit's first are code N, under which the zero state stays zero.  The key of section 15 step 2
//     -- the largest column in [jp - npad, jp] at which a real row holds `value`, the smallest such row, and whether column jp
//     attains `value` (a real row there, or row m - 1 in one of those columns: a pad row's echo) -- is looked for in the last
//     two groups only (a uniform branch), by a walk over the registers after the column;
//   * pass (ii): the anchored matrix from (i1, j1) towards smaller rows and columns until a column holds a pair that scores
//     `value`: at most min(j1 + 1, W(m)) columns.  Lanes finish at different columns; the wave loops until all have.
//
// The output is k_site_ends' SiteAlignEnds, word for word; pass (iii) is k_site_path as it is.  No scratch, no atomics, plain
// vector stores: ends[p] has one writer, lane p.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "kernels.h"

namespace fasim {

int site_short_warm(int m) { return (scan_short_warmup(m) + 16 + 15) & ~15; }

namespace {

constexpr int SSH_NEG = -(1 << 20);              // "no path": -2^20 - 16 * 516 does not wrap, -2^20 + 5 * 516 is no value
constexpr int SSH_NONE = 1 << 20;                // a row / a value that does not exist
constexpr uint32_t SSH_N4 = 0x04040404u;         // four columns of code N

template <int ROWS>
__global__ void __launch_bounds__(256) k_site_ends_short(SiteEndsLaunch a, int warm, int wmax)
{
	__shared__ int prof[ROWS * 5];                // [row][target code]: +5 / -4; pad rows -4 (they are computed and never looked at)
	__shared__ int qrev[2 * ROWS];                // [ROWS guard entries of code N][the oligo's codes, padded with N]
	const int m = a.m;
	for (int idx = threadIdx.x; idx < ROWS * 5; idx += 256) {
		const int row = idx / 5, code = idx - row * 5;
		const int q = row < m ? (int)a.qcodes[row] : 4;
		prof[idx] = (q == code && code < 4) ? 5 : -4;
	}
	for (int idx = threadIdx.x; idx < 2 * ROWS; idx += 256) qrev[idx] = (idx >= ROWS && idx - ROWS < m) ? (int)a.qcodes[idx - ROWS] : 4;
	__syncthreads();

	const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const bool mine = p < a.nprob;
	SiteAlignProb P; P.tbase = 0; P.n = 0; P.jp = 0; P.value = 0; P.pad = 0;
	if (mine) P = a.probs[p];
	const bool ok = mine && P.n >= 1 && P.jp >= 0 && P.jp < P.n && P.value >= 1;
	const int jp = ok ? P.jp : 0, value = ok ? P.value : SSH_NONE;
	const uint8_t* tc = a.tcodes + (ok ? P.tbase : 0);

	int H[ROWS], E[ROWS];
#pragma unroll
	for (int i = 0; i < ROWS; i++) { H[i] = 0; E[i] = 0; }

	// ---- pass (i): the local matrix over the window, the key of the end cell in its last columns
	const int c_lo = max(0, jp - a.npad), g0 = (jp & ~15) - warm, ngroups = warm / 16 + 1;
	int i1 = -1, j1 = -1, att = 0;
#pragma unroll 1
	for (int g = 0; g < ngroups; g++) {
		const int cA = g0 + 16 * g;               // a multiple of 16, at most jp: the group lies inside the unit's padded row or before it
		uint4 w = make_uint4(SSH_N4, SSH_N4, SSH_N4, SSH_N4);
		if (ok && cA >= 0) w = *reinterpret_cast<const uint4*>(tc + cA);
		const bool track = g >= ngroups - 2;      // (uniform) [jp - 15, jp] lies in the last two groups
#pragma unroll 1
		for (int k = 0; k < 16; k++) {
			const int* pr = prof + min(w.x & 0xffu, 4u);
			w.x = __builtin_amdgcn_alignbit(w.y, w.x, 8); w.y = __builtin_amdgcn_alignbit(w.z, w.y, 8);
			w.z = __builtin_amdgcn_alignbit(w.w, w.z, 8); w.w >>= 8;
			int hd = 0, f = SSH_NEG, hn = 0;
#pragma unroll
			for (int i = 0; i < ROWS; i++) {
				const int hc = H[i];
				const int e = max(E[i] - 4, hc - 16);
				if (i > 0) f = max(f - 4, hn - 16);
				const int h = max(max(hd + pr[i * 5], e), max(f, 0));
				H[i] = h; E[i] = e; hd = hc; hn = h;
			}
			if (track) {
				const int c = cA + k;
				int row = -1, last = 0;
#pragma unroll
				for (int i = ROWS - 1; i >= 0; i--) {
					// (rows below ROWS - 16 are real for every m of this build: only the last 16 ask)
					const bool hit = H[i] == value && (i < ROWS - 16 || i < m);
					row = hit ? i : row;
					if (i >= ROWS - 16) last = (hit && i == m - 1) ? 1 : last;
				}
				if (row >= 0 && c >= c_lo && c <= jp) { j1 = c; i1 = row; att |= (c == jp) | last; }
			}
		}
	}
	if (!att) { i1 = -1; j1 = -1; }

	// ---- pass (ii): the anchored matrix from the end cell, row r = query row i1 - r, column c = target column j1 - c
	int i0 = -1, j0 = -1;
	const bool has_end = i1 >= 0;
	const int cols = has_end ? min(j1 + 1, wmax) : 0;
	const int* qb = qrev + ROWS + (has_end ? i1 : 0);
	const uint8_t* tcol = tc + (has_end ? j1 : 0);
	bool live = cols > 0;
#pragma unroll
	for (int i = 0; i < ROWS; i++) { H[i] = SSH_NEG; E[i] = SSH_NEG; }
#pragma unroll 1
	for (int c = 0; __any(live); c++) {
		int tcode = 4;
		if (live) tcode = min((int)tcol[-c], 4);
		const int sel = tcode < 4 ? tcode : -1;   // a query code equal to `sel` scores +5
		int hd = c == 0 ? 0 : SSH_NEG, f = SSH_NEG, hn = SSH_NEG, hitrow = SSH_NONE;
#pragma unroll
		for (int i = 0; i < ROWS; i++) {
			const int hc = H[i];
			const int e = max(E[i] - 4, hc - 16);
			if (i > 0) f = max(f - 4, hn - 16);
			const int dg = hd + (qb[-i] == sel ? 5 : -4);
			const int h = max(max(dg, e), f);
			hitrow = min(hitrow, dg == value ? i : SSH_NONE);
			H[i] = h; E[i] = e; hd = hc; hn = h;
		}
		if (live) {
			if (hitrow <= i1) { j0 = j1 - c; i0 = i1 - hitrow; live = false; }
			else if (c + 1 >= cols) live = false;
		}
	}
	if (mine) *reinterpret_cast<int4*>(&a.ends[p]) = make_int4(i1, j1, i0, j0);
}

template <int ROWS>
hipError_t sse_launch(const SiteEndsLaunch& L, hipStream_t st)
{
	hipLaunchKernelGGL(k_site_ends_short<ROWS>, dim3((unsigned)((L.nprob + 255) / 256)), dim3(256), 0, st, L, site_short_warm(L.m), scan_short_warmup(L.m));
	return hipGetLastError();
}

} // namespace

hipError_t launch_site_ends_short(const SiteEndsLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (L.m < 1 || L.m > SCAN_SHORT_MAX || L.npad != 16 * ((L.m + 15) / 16) - L.m || !L.tcodes || !L.qcodes || !L.probs || !L.ends) return hipErrorInvalidValue;
	switch ((L.m + 15) / 16) {
	case 1: return sse_launch<16>(L, st);
	case 2: return sse_launch<32>(L, st);
	case 3: return sse_launch<48>(L, st);
	case 4: return sse_launch<64>(L, st);
	case 5: return sse_launch<80>(L, st);
	case 6: return sse_launch<96>(L, st);
	default: return sse_launch<112>(L, st);
	}
}

} // namespace fasim
