// fasim-longtarget_amd/csrc/mutagenesis.hip -- every substitution at every position of an interval, scored by the triplex potential
// through it, from one shared pass, for gfx950.
//
// The problems of an interval -- position x, letter b, encoding e -- are section 19's touching matrix T over one context, the interval
// and its flanks, with one column exchanged.  Left of that column T is the plain local recurrence on the context's own letters,
// whichever x and b: k_mut_prefix runs it once per (context, encoding) and stores the row state before every column of the interval,
// the snapshots.  k_mut_touch starts a problem from its snapshot: the exchanged column in plain mode, then the context's columns with
// the diagonal that only continues, and it stops with the first column in which every H and E of the real rows is zero: nothing starts
// afresh behind the allele, so every later column is zero too.  k_mut_reduce folds the problems of a position into twenty words.
//
// The column step is colstep.h's, cell for cell k_touch's (variant.hip): one workgroup of touch_threads(m) threads per unit or
// problem, the 16-bit row state in LDS or, for queries above TOUCH_LDS_ROWS rows, in HBM, every value carried as 2 * value + clip bit.
// The four letters of a position are four workgroups, not one workgroup in turn: each stops at its own dead column (the test is
// uniform per workgroup), there are four times as many workgroups to fill the device with, and what one in turn would save, three
// loads of a snapshot, is 4 bytes per row against some ninety columns of work on it.
// No atomics on global memory, plain vector stores only; every output word has one writer.
// Behind them, on the same column and the same snapshots: every deletion of an interval (section 27; k_mut_prefix_pm, k_mut_jump,
// k_mut_del_reduce).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "colstep.h"

namespace fasim {

constexpr int MT_THREADS = 256;

// One column of T over the thread's rows, k_touch's two walks.  Leaves H in nxt and E in S.e, takes the real rows' H into best where
// `counts`, and returns whether a real row of the thread has H or E above zero.  The caller's barrier follows.
template <int NT, bool IN_LDS>
__device__ __forceinline__ int mut_column(ColState<NT, IN_LDS>& S, const uint16_t* cur, uint16_t* nxt, int tcode, bool cont, int mark, bool counts,
	int& best, int* wtot)
{
	const int t = S.t, rpt = S.rpt;
	const int top = t > 0 ? (int)cur[S.above] : 0;      // H of the previous column in the row above the thread's first
	int hd = top, f = 0, hn = 0, live = 0;
	for (int i0 = 0; i0 < rpt; i0 += COL_UNROLL) {
		int hc[COL_UNROLL], ein[COL_UNROLL], sc[COL_UNROLL];
		col_load<2>(S, cur, i0, tcode, hc, ein, sc);
#pragma unroll
		for (int k = 0; k < COL_UNROLL; k++) if (i0 + k < rpt) {
			int e, h = col_cell<2>(hd, hc[k], ein[k], sc[k], cont, i0 + k > 0, hn, f, e);
			if (mark && h) h |= 1;
			if (i0 + k < S.cnt) { live |= h | e; if (counts) best = max(best, h); }
			nxt[S.at(i0 + k)] = (uint16_t)h; S.e[S.at(i0 + k)] = (uint16_t)e;
			hd = hc[k]; hn = h;
		}
	}
	const int fin = col_gap_in<2>(S, col_gap<2>(f, hn), wtot);
	// second walk, where a gap enters a thread of the wave from above: H = max(H, the gap continued from fin)
	if (__any(fin > 0)) {
		f = fin;
		for (int i = 0; i < rpt; i++) {
			if (i > 0) f = col_floor<2>(col_gap<2>(f, hn));
			const int h = max((int)nxt[S.at(i)], f);      // (f carries the bit of the marked cell it comes from)
			if (i < S.cnt) { live |= h; if (counts) best = max(best, h); }
			nxt[S.at(i)] = (uint16_t)h;
			hn = h;
		}
	}
	return live;
}

__device__ __forceinline__ bool mut_unit_ok(const TouchProb& P) { return P.n >= 1 && P.n <= TOUCH_MAX_COLS && P.v0 >= 0 && P.v0 < P.v1 && P.v1 <= P.n; }

// One workgroup of NT threads per unit: the plain recurrence over the columns before v1 - 1, the row state before every column of
// [v0, v1) out
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_mut_prefix(MutLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char mt_lds[];
	__shared__ int wtot[4];
	const int u = blockIdx.x;
	if (u >= a.nunit) return;
	const TouchProb P = a.units[u];
	ColState<NT, IN_LDS> S;
	S.open(mt_lds, lds_rows, a.rows, u, a.qcodes, a.m);
	__syncthreads();
	if (!mut_unit_ok(P)) return;      // (uniform)
	const int rpt = S.rpt;
	const int64_t words = (int64_t)rpt * NT;
	uint16_t* snap = a.snap + (int64_t)a.first[u] * 2 * words;
	const uint8_t* tc = a.tcodes + P.tbase;
	int best = 0;
	for (int c = 0; c < P.v1; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		if (c >= P.v0) {      // the thread's own rows, which it wrote itself
			uint16_t* d = snap + (int64_t)(c - P.v0) * 2 * words;
			for (int i = 0; i < rpt; i++) { d[S.at(i)] = cur[S.at(i)]; d[words + S.at(i)] = S.e[S.at(i)]; }
		}
		if (c == P.v1 - 1) break;      // nothing behind the last snapshot is wanted
		(void)mut_column(S, cur, nxt, tc[c], false, (c == 0 && (P.edge & 1)) ? 1 : 0, false, best, wtot);
		__syncthreads();
	}
}

// One workgroup of NT threads per problem (column, letter)
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_mut_touch(MutLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char mt_lds[];
	__shared__ int wtot[4];
	__shared__ unsigned best_sh;
	const int p = blockIdx.x;
	if (p >= 4 * a.ncol) return;
	const int g = p >> 2, letter = p & 3;
	int lo = 0, hi = a.nunit - 1;      // the last unit with first[u] <= g
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.first[mid] <= g) lo = mid; else hi = mid - 1; }
	const int u = lo;
	const TouchProb P = a.units[u];
	const int c0 = P.v0 + (g - a.first[u]);
	ColState<NT, IN_LDS> S;
	S.open(mt_lds, lds_rows, a.rows, p, a.qcodes, a.m);
	const int t = S.t, rpt = S.rpt;
	const bool ok = mut_unit_ok(P) && c0 >= P.v0 && c0 < P.v1;      // (uniform)
	if (ok) {      // the snapshot into the row state before column c0: the thread's own rows
		const int64_t words = (int64_t)rpt * NT;
		const uint16_t* sn = a.snap + (int64_t)g * 2 * words;
		uint16_t* cur = (c0 & 1) ? S.h[1] : S.h[0];
		for (int i = 0; i < rpt; i++) { cur[S.at(i)] = sn[S.at(i)]; S.e[S.at(i)] = sn[words + S.at(i)]; }
	}
	if (t == 0) best_sh = 0;
	__syncthreads();
	const uint8_t* tc = a.tcodes + P.tbase;
	const int lcode = a.enc_lut[P.enc * 256 + "ACGT"[letter]];
	int best = 0, ran = 0;
	for (int c = c0; ok && c < P.n; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const int mark = ((c == 0 && (P.edge & 1)) || (c == P.n - 1 && (P.edge & 2))) ? 1 : 0;
		// behind the allele's column the diagonal only continues an alignment
		const int live = mut_column(S, cur, nxt, c == c0 ? lcode : (int)tc[c], c > c0, mark, true, best, wtot);
		ran++;
		if (!__syncthreads_or(live)) break;      // a dead column: every later one is dead
	}
	if (best) atomicMax(&best_sh, (unsigned)best);      // (LDS)
	__syncthreads();
	if (t == 0) { a.out[p] = best_sh; a.cols[p] = (uint32_t)ran; }
}

__device__ __forceinline__ int mt_class(int enc) { return enc < 12 ? (enc & 1) : (((enc - 12) & 1) ? 3 : 2); }

// one thread per (position, letter) of the launch
__global__ void __launch_bounds__(MT_THREADS) k_mut_reduce(MutReduceLaunch a)
{
	const int idx = blockIdx.x * MT_THREADS + threadIdx.x;
	const int pos = idx >> 2, letter = idx & 3;
	if (pos >= a.npos) return;
	int lo = 0, hi = a.ngroup - 1;      // the last group with pos0 <= pos
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.groups[mid].pos0 <= pos) lo = mid; else hi = mid - 1; }
	const MutGroup G = a.groups[lo];
	const int j = pos - G.pos0;
	if (j < 0 || j >= G.npos) return;
	uint32_t* o = a.out + (int64_t)pos * MUT_WORDS;
	unsigned ran = 0;
	for (int cls = 0; cls < 4; cls++) {
		unsigned bx = 0, be = 0xff;
		for (int k = 0; k < a.nenc; k++) {
			const int enc = a.enc[k];
			if (mt_class(enc) != cls) continue;
			const int64_t prob = ((int64_t)a.first[G.unit0 + k] + ((enc & 1) ? G.npos - 1 - j : j)) * 4 + letter;
			const unsigned w = a.touch[prob];
			ran += a.cols[prob];
			if ((w >> 1) > (bx >> 1)) be = (unsigned)enc;      // (the encodings come in ascending order)
			bx = max(bx, w);
		}
		o[letter * 4 + cls] = (bx << 8) | be;
	}
	o[16 + letter] = ran;
}

static bool mut_launch_ok(const MutLaunch& L)
{
	return L.m >= 1 && L.tcodes && L.qcodes && L.units && L.first && L.enc_lut && L.snap && L.out && L.cols && L.ncol >= L.nunit && L.ncol <= (1 << 28);
}

hipError_t launch_mut_prefix(const MutLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (!mut_launch_ok(L)) return hipErrorInvalidValue;
	return launch_cols(L, L.nunit, st, [](auto nt, auto lds) { return k_mut_prefix<decltype(nt)::value, decltype(lds)::value>; });
}

hipError_t launch_mut_touch(const MutLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (!mut_launch_ok(L)) return hipErrorInvalidValue;
	return launch_cols(L, 4 * L.ncol, st, [](auto nt, auto lds) { return k_mut_touch<decltype(nt)::value, decltype(lds)::value>; });
}

hipError_t launch_mut_reduce(const MutReduceLaunch& L, hipStream_t st)
{
	if (L.npos <= 0) return hipSuccess;
	if (!L.touch || !L.cols || !L.first || !L.groups || !L.out || L.ngroup < 1 || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_mut_reduce, dim3((unsigned)(((int64_t)L.npos * 4 + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, st, L);
	return hipGetLastError();
}

// ---- every deletion of an interval ---------------------------------------------------------------------------
// A deletion (x, d) keeps base x and takes the d bases behind it out.  Its REF problem marks d + 1 columns of the context: the value
// is the maximum over the plain column maxima of the first d of them -- k_mut_prefix_pm writes those beside the snapshots -- and the
// own-letter problem of the last, which is the same for every deletion that ends there.  Its ALT problem runs the anchor's column and
// goes on behind the deleted run from the row state before the anchor (even) or before the run (odd, where the run comes first and
// the anchor's column is the mark's last).
// Both are jump problems of k_mut_jump; k_mut_del_reduce folds them into ten words per (position, length).

// the last unit with first[u] <= g
__device__ __forceinline__ int del_unit_of(const int32_t* first, int nunit, int g)
{
	int lo = 0, hi = nunit - 1;
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= g) lo = mid; else hi = mid - 1; }
	return lo;
}

__device__ __forceinline__ bool del_group_ok(const DelGroup& G, const TouchProb& P, int nunit, int nenc)
{
	return mut_unit_ok(P) && G.npos >= 1 && G.npos <= G.next && G.next == P.v1 - P.v0 && G.unit0 >= 0 && G.unit0 + nenc <= nunit;
}

// k_mut_prefix, and the column maxima of the columns [v0, v1 - 1) out: every thread's maximum into one of two LDS words by the
// column's parity, the column's barrier, one store by thread 0, which also clears the word for the column after the next
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_mut_prefix_pm(DelLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char mt_lds[];
	__shared__ int wtot[4];
	__shared__ unsigned top_sh[2];
	const int u = blockIdx.x;
	if (u >= a.nunit) return;
	const TouchProb P = a.units[u];
	ColState<NT, IN_LDS> S;
	S.open(mt_lds, lds_rows, a.rows, u, a.qcodes, a.m);
	if (S.t < 2) top_sh[S.t] = 0;
	__syncthreads();
	if (!mut_unit_ok(P)) return;      // (uniform)
	const int rpt = S.rpt;
	const int64_t words = (int64_t)rpt * NT;
	const int64_t g0 = a.first[u];
	uint16_t* snap = a.snap + g0 * 2 * words;
	const uint8_t* tc = a.tcodes + P.tbase;
	for (int c = 0; c < P.v1; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const bool inside = c >= P.v0;
		if (inside) {      // the thread's own rows, which it wrote itself
			uint16_t* d = snap + (int64_t)(c - P.v0) * 2 * words;
			for (int i = 0; i < rpt; i++) { d[S.at(i)] = cur[S.at(i)]; d[words + S.at(i)] = S.e[S.at(i)]; }
		}
		if (c == P.v1 - 1) break;      // nothing behind the last snapshot is wanted
		int best = 0;
		(void)mut_column(S, cur, nxt, tc[c], false, (c == 0 && (P.edge & 1)) ? 1 : 0, inside, best, wtot);
		if (best) atomicMax(&top_sh[c & 1], (unsigned)best);      // (LDS)
		__syncthreads();
		if (inside && S.t == 0) { a.pm[g0 + (c - P.v0)] = top_sh[c & 1]; top_sh[c & 1] = 0; }
	}
}

// One workgroup of NT threads per jump problem
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_mut_jump(DelLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char mt_lds[];
	__shared__ int wtot[4];
	__shared__ unsigned best_sh;
	const int p = blockIdx.x;
	if (p >= a.ncol + a.nalt) return;
	int u, s, k, r;
	bool ok;
	if (p < a.ncol) {      // the own-letter problem of snapshot column p
		u = del_unit_of(a.first, a.nunit, p);
		const TouchProb P = a.units[u];
		const DelGroup G = a.groups[u / a.nenc];
		const int c = P.v0 + (p - a.first[u]);
		const int j = (P.enc & 1) ? P.v1 - 1 - c : c - P.v0;
		// the last mark column of a REF problem: where a deletion of the group ends or, mirrored, where one is anchored
		bool used = (P.enc & 1) && j < G.npos && j + a.lengths[0] < G.next;
		for (int l = 0; l < a.nlen && !(P.enc & 1); l++) used |= j - a.lengths[l] >= 0 && j - a.lengths[l] < G.npos;
		ok = used && del_group_ok(G, P, a.nunit, a.nenc) && c < P.v1;
		s = c; k = c; r = c + 1;
	} else {      // the ALT problem of (position, length) under an encoding
		const int q = p - a.ncol;
		const int l = q % a.nlen, slot = q / a.nlen;
		int lo = 0, hi = a.ngroup - 1;      // the last group with pos0 * nenc <= slot
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.groups[mid].pos0 * a.nenc <= slot) lo = mid; else hi = mid - 1; }
		const DelGroup G = a.groups[lo];
		const int w = slot - G.pos0 * a.nenc, np = max(G.npos, 1);
		const int j = w % np, d = a.lengths[l];
		u = min(max(G.unit0 + w / np, 0), a.nunit - 1);
		const TouchProb P = a.units[u];
		ok = w >= 0 && w / np < a.nenc && j + d < G.next && del_group_ok(G, P, a.nunit, a.nenc);
		if (P.enc & 1) { k = P.v1 - 1 - j; s = k - d; r = k + 1; }
		else { k = P.v0 + j; s = k; r = k + 1 + d; }
	}
	const TouchProb P = a.units[u];
	ColState<NT, IN_LDS> S;
	S.open(mt_lds, lds_rows, a.rows, p, a.qcodes, a.m);
	const int t = S.t, rpt = S.rpt;
	if (ok) {      // the snapshot into the row state before column s: the thread's own rows
		const int64_t words = (int64_t)rpt * NT;
		const uint16_t* sn = a.snap + ((int64_t)a.first[u] + (s - P.v0)) * 2 * words;
		for (int i = 0; i < rpt; i++) { S.h[0][S.at(i)] = sn[S.at(i)]; S.e[S.at(i)] = sn[words + S.at(i)]; }
	}
	if (t == 0) best_sh = 0;
	__syncthreads();
	const uint8_t* tc = a.tcodes + P.tbase;
	int best = 0, ran = 0;
	for (int c = k; ok && c < P.n; c = ran == 1 ? r : c + 1) {
		const uint16_t* cur = (ran & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (ran & 1) ? S.h[0] : S.h[1];
		// the problem's first column is the context's if it starts from the state before column 0, its last the context's if nothing follows
		const int mark = ran == 0 ? (((s == 0 && (P.edge & 1)) || (r == P.n && (P.edge & 2))) ? 1 : 0) : ((c == P.n - 1 && (P.edge & 2)) ? 1 : 0);
		const int live = mut_column(S, cur, nxt, tc[c], ran > 0, mark, true, best, wtot);
		ran++;
		if (!__syncthreads_or(live)) break;      // a dead column: every later one is dead
	}
	if (best) atomicMax(&best_sh, (unsigned)best);      // (LDS)
	__syncthreads();
	if (t == 0) { a.out[p] = best_sh; a.cols[p] = (uint32_t)ran; }
}

// one thread per (position, length) of the launch
__global__ void __launch_bounds__(MT_THREADS) k_mut_del_reduce(DelLaunch a)
{
	const int64_t idx = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
	const int pos = (int)(idx / a.nlen), l = (int)(idx % a.nlen);
	if (pos >= a.npos) return;
	int lo = 0, hi = a.ngroup - 1;      // the last group with pos0 <= pos
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.groups[mid].pos0 <= pos) lo = mid; else hi = mid - 1; }
	const DelGroup G = a.groups[lo];
	const int j = pos - G.pos0, d = a.lengths[l];
	uint32_t* o = a.words + idx * DEL_WORDS;
	const bool valid = j >= 0 && j < G.npos && j + d < G.next;
	// an own-letter problem is counted once: at position j + d (even encodings) by the smallest length of the group that ends there,
	// at position j (odd encodings) by the smallest length
	const bool first_end = valid && (l == 0 || j + d - a.lengths[l - 1] >= G.npos), first_len = valid && l == 0;
	unsigned ran = 0;
	for (int al = 0; al < 2; al++) for (int cls = 0; cls < 4; cls++) {
		unsigned bx = 0, be = 0xff;
		for (int k = 0; valid && k < a.nenc; k++) {
			const int enc = a.enc[k];
			if (mt_class(enc) != cls) continue;
			const int64_t f = a.first[G.unit0 + k];
			unsigned w;
			if (al == 0) {      // REF: the column maxima of the first d mark columns and the own-letter problem of the last
				const int64_t own = (enc & 1) ? f + G.next - 1 - j : f + j + d;
				const int64_t m0 = (enc & 1) ? own - d : f + j;
				w = a.out[own];
				for (int x = 0; x < d; x++) w = max(w, a.pm[m0 + x]);
				if ((enc & 1) ? first_len : first_end) ran += a.cols[own];
			} else {
				const int64_t prob = (int64_t)a.ncol + (((int64_t)G.pos0 * a.nenc + (int64_t)k * G.npos + j) * a.nlen + l);
				w = a.out[prob];
				ran += a.cols[prob];
			}
			if ((w >> 1) > (bx >> 1)) be = (unsigned)enc;      // (the encodings come in ascending order)
			bx = max(bx, w);
		}
		o[al * 4 + cls] = (bx << 8) | be;
	}
	o[8] = ran;
	o[9] = valid ? 1u : 0u;
}

static bool del_launch_ok(const DelLaunch& L)
{
	if (!(L.m >= 1 && L.tcodes && L.qcodes && L.units && L.first && L.snap && L.pm && L.out && L.cols && L.groups && L.words)) return false;
	if (!(L.ngroup >= 1 && L.nenc >= 1 && L.nenc <= 48 && L.nunit == L.ngroup * L.nenc && L.ncol >= L.nunit && L.npos >= L.ngroup)) return false;
	if (!(L.nlen >= 1 && L.nlen <= 16 && (int64_t)L.nalt == (int64_t)L.npos * L.nenc * L.nlen && (int64_t)L.ncol + L.nalt <= (1 << 28))) return false;
	for (int l = 0; l < L.nlen; l++) if (L.lengths[l] < 1 || (l > 0 && L.lengths[l] <= L.lengths[l - 1])) return false;
	return true;
}

hipError_t launch_mut_prefix_pm(const DelLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (!del_launch_ok(L)) return hipErrorInvalidValue;
	return launch_cols(L, L.nunit, st, [](auto nt, auto lds) { return k_mut_prefix_pm<decltype(nt)::value, decltype(lds)::value>; });
}

hipError_t launch_mut_jump(const DelLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (!del_launch_ok(L)) return hipErrorInvalidValue;
	return launch_cols(L, L.ncol + L.nalt, st, [](auto nt, auto lds) { return k_mut_jump<decltype(nt)::value, decltype(lds)::value>; });
}

hipError_t launch_mut_del_reduce(const DelLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (!del_launch_ok(L)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_mut_del_reduce, dim3((unsigned)(((int64_t)L.npos * L.nlen + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
