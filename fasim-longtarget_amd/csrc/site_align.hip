// fasim-longtarget_amd/csrc/site_align.hip -- the hit of a site: the textbook local alignment behind its peak, for gfx950
// (DESIGN.md section 15).
//
// A site (sites.hip) is a range of DNA positions, a value, the position of the peak and an encoding.  Its hit is the alignment of
// score `value` that ends in the peak's column: end cell, start cell, CIGAR.  Three passes of one column-parallel Gotoh step:
//
//   k_site_ends, pass (i):   the local matrix H of section 11 over columns [0, jp] of the unit, all real rows (pad rows only
//                            repeat row m - 1 and feed nothing back, so they are not computed: their echo is looked for in row
//                            m - 1 of the npad columns before jp).  Leaves (i1, j1).
//   k_site_ends, pass (ii):  the anchored matrix from (i1, j1) towards smaller rows and columns (no floor, one starting cell),
//                            column by column until a column holds a pair that scores `value`.  Leaves (i0, j0).
//   k_site_path, pass (iii): the anchored matrix of the rectangle with one direction byte per cell, then the traceback by one lane.
//
// One 256-thread workgroup per problem.  A thread owns a contiguous block of query rows; the state of a row (H of the previous
// column, H of this column, E) is 16-bit in LDS, or in HBM for queries above SITE_ALIGN_LDS_ROWS rows; the arithmetic is 32-bit.
// A column is two walks of the thread's rows around a max-scan: the first walk leaves the vertical gap value the thread's rows
// hand to the row below them (opened in the thread's own rows; a gap never opens better from a cell that a gap reached), the scan
//   F_in(t) = max over t' < t of out(t') - 4 * rows * (t - 1 - t')
// gives every thread the gap value that enters its first row, and the second walk is the plain sequential recurrence from it.
// Passes (i) and (ii) scan with colstep.h's scan_excl; pass (iii) also needs to know whether the entering gap was
// extended or opened in the row above, so there every thread folds the (at most 256) outputs before it from LDS in order.
// No atomics on global memory, plain vector stores only; every output word has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "colstep.h"

namespace fasim {

constexpr int SA_THREADS = 256;
constexpr int SA_NEG = -30000;                 // "no alignment" in the 16-bit state (real scores of a path stay above -16 384); safe for units of at most SITE_ALIGN_MAX_COLS columns: -30 000 + 5 * 6 000 < 1 and 5 * 6 000 < 32 767

struct SaState {
	int16_t* h[2];                              // [rows]: H of the previous / this column, swapped every column
	int16_t* e;                                 // [rows]
	const uint8_t* q;                           // query codes in natural order (LDS copy or HBM)
};

__device__ __forceinline__ int16_t sa_store(int x) { return (int16_t)min(max(x, SA_NEG), 32767); }

// MODE 0: local (floored at 0), forward: rows 0 .. R - 1 are query rows q0 + r, columns 0 .. C - 1 target columns t0 + c.
//         Result: res[0] = key of the end cell ((column - c_lo + 1) << 20 | (0xfffff - row), 0: none), res[1] = the unit attains
//         `value` in its last column (a real row there, or row R - 1 in one of the columns from c_lo on: a pad row's echo).
// MODE 1: anchored, reversed: row r is query row q0 - r, column c target column t0 - c; stops at the first column that holds a
//         pair scoring `value`.  Result: res[0] = that column (-1: none), res[1] = its smallest row.
// MODE 2: anchored, forward, direction bytes to dirs[c * R + r] (bits 0-1: H from 0 diagonal / 1 E / 2 F; bit 2: E extended; bit 3:
//         F extended).  Result: res[0] = H of the last cell.
// sh: 8 + 2 * SA_THREADS words of LDS.  Every thread of the workgroup calls it with the same arguments.
template <int MODE>
__device__ void sa_pass(const SaState& S, const uint8_t* tc, int t0, int q0, int R, int C, int value, int c_lo, uint8_t* dirs, int* sh,
	int res[2])
{
	constexpr int DIR = MODE == 1 ? -1 : 1;
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int rpt = (R + SA_THREADS - 1) / SA_THREADS;
	const int first = min(R, t * rpt), last = min(R, first + rpt);
	int* wtot = sh;                              // [4]
	int* red = sh + 4;                           // [4]: results
	int* outa = sh + 8;                          // [SA_THREADS] MODE 2: the gap value a thread's rows hand down by extension
	int* outb = outa + SA_THREADS;               // [SA_THREADS] MODE 2: ... by opening in its last row
	const int init = MODE == 0 ? 0 : SA_NEG;
	for (int r = first; r < last; r++) { S.h[0][r] = (int16_t)init; S.e[r] = (int16_t)init; }
	if (t == 0) { red[0] = MODE == 1 ? 0x7fffffff : 0; red[1] = 0; red[2] = SA_NEG; red[3] = 0; }
	__syncthreads();
	unsigned key = 0; int att = 0;
	for (int c = 0; c < C; c++) {
		const int16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		int16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const int tcode = tc[t0 + DIR * c];
		const int top = MODE == 0 ? 0 : (c == 0 ? 0 : SA_NEG);      // the diagonal neighbour of row 0
		// first walk: what the thread's own rows hand down
		int oa = NEG32, ob = NEG32;
		if (first < last) {
			int hd = first == 0 ? top : (int)cur[first - 1];
			int f = NEG32, hn = 0;
			for (int r = first; r < last; r++) {
				const int hc = cur[r];
				const int e = max((int)S.e[r] - 4, hc - 16);
				if (r > first) f = max(f - 4, hn - 16);
				int h = max(max(hd + col_score<1>(S.q[q0 + DIR * r], tcode), e), f);
				if (MODE == 0) h = max(h, 0);
				hd = hc; hn = h;
			}
			oa = f - 4; ob = hn - 16;
		}
		int fin, fin_ext = 0;
		if (MODE == 2) {
			outa[t] = oa; outb[t] = ob;
			__syncthreads();
			const int nact = (R + rpt - 1) / rpt;
			fin = NEG32;
			for (int k = 0; k < nact; k++) {
				if (k >= t) break;
				const int ext = max(fin - 4 * rpt, outa[k]), opn = outb[k];
				fin = max(ext, opn); fin_ext = ext >= opn;
			}
		} else {
			const int ex = scan_excl<SA_THREADS>(max(oa, ob) + 4 * rpt * t, wtot, lane, wave);
			fin = t == 0 ? NEG32 : ex - 4 * rpt * (t - 1);
		}
		fin = max(fin, NEG32);
		// second walk: the recurrence itself
		int hit = 0, hit_row = 0x7fffffff;
		if (first < last) {
			int hd = first == 0 ? top : (int)cur[first - 1];
			int f = fin, hn = 0;
			for (int r = first; r < last; r++) {
				const int hc = cur[r], eo = S.e[r];
				const int e = max(eo - 4, hc - 16);
				int fext = fin_ext;
				if (r > first) { fext = f - 4 >= hn - 16; f = max(f - 4, hn - 16); }
				const int dg = hd + col_score<1>(S.q[q0 + DIR * r], tcode);
				int h = max(max(dg, e), f);
				if (MODE == 0) h = max(h, 0);
				if (MODE == 0) {
					if (c >= c_lo && h == value) {
						key = max(key, ((unsigned)(c - c_lo + 1) << 20) | (unsigned)(0xfffff - r));
						att |= (c == C - 1 || r == R - 1);
					}
				}
				if (MODE == 1) { if (dg == value && !hit) { hit = 1; hit_row = r; } }
				if (MODE == 2) {
					const int src = h == dg ? 0 : (h == e ? 1 : 2);
					dirs[(int64_t)c * R + r] = (uint8_t)(src | ((e == eo - 4) ? 4 : 0) | (fext ? 8 : 0));
					if (c == C - 1 && r == R - 1) red[2] = h;
				}
				nxt[r] = sa_store(h); S.e[r] = sa_store(e);
				hd = hc; hn = h;
			}
		}
		if (MODE == 1) {
			if (__syncthreads_or(hit)) {
				if (hit) atomicMin(&red[0], hit_row);      // (LDS)
				__syncthreads();
				res[0] = c; res[1] = red[0];
				return;
			}
		} else __syncthreads();
	}
	if (MODE == 0) {
		if (key) atomicMax((unsigned*)&red[0], key);      // (LDS)
		if (att) atomicOr(&red[1], 1);
		__syncthreads();
		res[0] = red[0]; res[1] = red[1];
	} else if (MODE == 1) { res[0] = -1; res[1] = -1; }
	else { __syncthreads(); res[0] = red[2]; res[1] = 0; }
}

// dynamic LDS: [lds_rows] x (3 x int16 + 1 code byte), lds_rows = 0: the row state lives in a.rows and the codes are read from HBM
__global__ void __launch_bounds__(SA_THREADS) k_site_ends(SiteEndsLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char sa_lds[];
	__shared__ int sh[8 + 2 * SA_THREADS];
	const int p = blockIdx.x;
	if (p >= a.nprob) return;
	const SiteAlignProb P = a.probs[p];
	const int m = a.m;
	SaState S;
	if (lds_rows > 0) {
		int16_t* b = reinterpret_cast<int16_t*>(sa_lds);
		S.h[0] = b; S.h[1] = b + lds_rows; S.e = b + 2 * lds_rows;
		uint8_t* qc = reinterpret_cast<uint8_t*>(b + 3 * lds_rows);
		for (int i = threadIdx.x; i < m; i += SA_THREADS) qc[i] = a.qcodes[i];
		S.q = qc;
	} else {
		int16_t* b = a.rows + (int64_t)p * 3 * m;
		S.h[0] = b; S.h[1] = b + m; S.e = b + 2 * m;
		S.q = a.qcodes;
	}
	__syncthreads();
	SiteAlignEnds out = { -1, -1, -1, -1 };
	const bool ok = P.n >= 1 && P.jp >= 0 && P.jp < P.n && P.value >= 1;      // (uniform)
	if (ok) {
		const uint8_t* tc = a.tcodes + P.tbase;
		const int c_lo = max(0, P.jp - a.npad);
		int res[2];
		sa_pass<0>(S, tc, 0, 0, m, P.jp + 1, P.value, c_lo, nullptr, sh, res);
		if (res[0] != 0 && res[1] != 0) {
			const unsigned key = (unsigned)res[0];
			out.j1 = c_lo + (int)(key >> 20) - 1; out.i1 = 0xfffff - (int)(key & 0xfffff);
			__syncthreads();
			sa_pass<1>(S, tc, out.j1, out.i1, out.i1 + 1, out.j1 + 1, P.value, 0, nullptr, sh, res);
			if (res[0] >= 0) { out.j0 = out.j1 - res[0]; out.i0 = out.i1 - res[1]; }
		}
	}
	if (threadIdx.x == 0) *reinterpret_cast<int4*>(&a.ends[p]) = make_int4(out.i1, out.j1, out.i0, out.j0);
}

__global__ void __launch_bounds__(SA_THREADS) k_site_path(SitePathLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char sa_lds[];
	__shared__ int sh[8 + 2 * SA_THREADS];
	const int k = blockIdx.x;
	if (k >= a.nitem) return;
	const SitePathItem I = a.items[k];
	const SiteAlignProb P = a.probs[I.prob];
	const int R = I.i1 - I.i0 + 1, C = I.j1 - I.j0 + 1;
	// (uniform) the host sized the LDS, the direction bytes and the CIGAR for exactly this rectangle
	if (R < 1 || C < 1 || R > lds_rows || I.i0 < 0 || I.j0 < 0 || I.j1 >= P.n || I.cig_cap < 1) { if (threadIdx.x == 0) a.cigar_len[k] = -1; return; }
	SaState S;
	int16_t* b = reinterpret_cast<int16_t*>(sa_lds);
	S.h[0] = b; S.h[1] = b + lds_rows; S.e = b + 2 * lds_rows;
	S.q = a.qcodes;
	uint8_t* dirs = a.dirs + I.dir_off;
	int res[2];
	sa_pass<2>(S, a.tcodes + P.tbase, I.j0, I.i0, R, C, P.value, 0, dirs, sh, res);
	if (threadIdx.x != 0) return;
	// traceback by one lane (the direction bytes of the workgroup are visible after the barrier that ended the pass)
	int len = -1;
	if (res[0] == P.value) {
		CigarRun cig(a.cigar + I.cig_off, I.cig_cap);
		int r = R - 1, c = C - 1, state = 0;
		bool bad = false;
		for (int step = 0; step < 2 * (R + C) + 4; step++) {
			if (r < 0 || c < 0) { bad = !(r == -1 && c == -1 && state == 0); break; }
			const int d = dirs[(int64_t)c * R + r];
			int op;
			if (state == 0) {
				const int src = d & 3;
				if (src == 1) { state = 1; continue; }
				if (src == 2) { state = 2; continue; }
				op = 0; r--; c--;
			} else if (state == 1) { op = 2; if (!(d & 4)) state = 0; c--; }
			else { op = 1; if (!(d & 8)) state = 0; r--; }
			if (!cig.push(op)) { bad = true; break; }
		}
		if (!bad && !(r == -1 && c == -1 && state == 0)) bad = true;
		if (!bad && !cig.flush()) bad = true;
		len = bad ? -1 : cig.nops;
	}
	a.cigar_len[k] = len;
}

hipError_t launch_site_ends(const SiteEndsLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (L.m < 1 || L.m > 0xfffff || L.npad < 0 || L.npad > 15 || !L.tcodes || !L.qcodes || !L.probs || !L.ends) return hipErrorInvalidValue;
	const bool lds = L.m <= SITE_ALIGN_LDS_ROWS;
	if (!lds && !L.rows) return hipErrorInvalidValue;
	const int lds_rows = lds ? ((L.m + 7) & ~7) : 0;
	hipLaunchKernelGGL(k_site_ends, dim3((unsigned)L.nprob), dim3(SA_THREADS), lds ? lds_bytes(lds_rows) : 0, st, L, lds_rows);
	return hipGetLastError();
}

// every rectangle of the launch has at most L.max_rows <= SITE_ALIGN_LDS_ROWS rows (the caller leaves taller ones unaligned)
hipError_t launch_site_path(const SitePathLaunch& L, hipStream_t st)
{
	if (L.nitem <= 0) return hipSuccess;
	if (!L.tcodes || !L.qcodes || !L.probs || !L.items || !L.dirs || !L.cigar || !L.cigar_len) return hipErrorInvalidValue;
	if (L.max_rows < 1 || L.max_rows > SITE_ALIGN_LDS_ROWS) return hipErrorInvalidValue;
	const int lds_rows = (L.max_rows + 7) & ~7;
	hipLaunchKernelGGL(k_site_path, dim3((unsigned)L.nitem), dim3(SA_THREADS), (size_t)lds_rows * 6, st, L, lds_rows);      // (three 16-bit words per row: the query codes are read from HBM)
	return hipGetLastError();
}

} // namespace fasim
