// fasim-longtarget_amd/csrc/variant.hip -- the triplex potential through a variant: per allele window and encoding the best local
// alignment that touches the allele's columns, for gfx950.
//
// A problem is one allele window (flank, allele, flank) under one encoding: n <= TOUCH_MAX_COLS target codes and the allele's columns
// [v0, v1).  k_touch runs the touching matrix T over all m real rows of the query: the plain local Gotoh recurrence of section 11 in
// the columns before v1, and from v1 on the same recurrence with a diagonal that only continues (Hdiag > 0 ? Hdiag + s : 0), so that
// nothing starts afresh behind the allele.  The result is the maximum of T over the columns from v0 on.  Every value is carried as
// 2 * value + b (scores and gap costs doubled): b, the clip bit, is set on the positive cells of a first or last column that the flank
// cut and travels through every maximum and every add; 0 means "no alignment" and carries no bit.
//
// The column step is the one of site_align.hip, passes (i) and (ii): one workgroup of 256 threads per problem (64 or 128 for queries of
// at most that many rows), a thread owns a contiguous block of query rows, a column is a walk of the thread's rows, an exclusive
// max-scan (__shfl_up and one LDS word per wave) of the vertical gap value the thread hands down, and a second walk that continues the
// gap that enters from above.  The state of a row (H of the previous column, H of this column, E) is 16-bit, unsigned here, in LDS or,
// for queries above TOUCH_LDS_ROWS rows, in HBM; the arithmetic is 32-bit.
// k_var_encode assembles and encodes the windows from the record on the device; k_touch_reduce folds the problems of a variant into
// nine words.  No atomics on global memory, plain vector stores only; every output word has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

constexpr int VT_THREADS = 256;
constexpr int VT_NEG32 = -(1 << 28);           // "nothing handed down" in the scan

struct VtState {
	uint16_t* h[2];                             // [rows]: H of the previous / this column, swapped every column
	uint16_t* e;                                // [rows]
	const uint8_t* q;                           // query codes (LDS copy or HBM)
};

__device__ __forceinline__ int vt_score2(int qc, int tc) { return (qc == tc && tc < 4) ? 10 : -8; }
__device__ __forceinline__ int vt_floor(int x) { return x < 2 ? 0 : x; }      // value 0: no alignment, no bit

constexpr int VT_UNROLL = 4;                   // rows whose state is loaded ahead of their cells

// exclusive max-scan of b over the NT threads of the workgroup (thread order); wtot: one word of LDS per wave.  Contains one
// __syncthreads where the workgroup has more than one wave.
template <int NT>
__device__ __forceinline__ int vt_scan_excl(int b, int* wtot, int lane, int wave)
{
	int inc = b;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int x = __shfl_up(inc, d);
		if (lane >= d) inc = max(inc, x);
	}
	int ex = __shfl_up(inc, 1);
	if (lane == 0) ex = VT_NEG32;
	if (NT > 64) {
		if (lane == 63) wtot[wave] = inc;
		__syncthreads();
		for (int w = 0; w < wave; w++) ex = max(ex, wtot[w]);
	}
	return ex;
}

// tcodes[tbase + c], c in [0, n): the code of window letter c (n - 1 - c for an odd encoding) under the problem's encoding
__global__ void __launch_bounds__(VT_THREADS) k_var_encode(VarEncodeLaunch a)
{
	const int p = blockIdx.x;
	if (p >= a.nprob) return;
	const TouchProb P = a.probs[p];
	const VarWindow W = a.wins[P.win];
	const uint8_t* lut = a.enc_lut + P.enc * 256;
	const uint8_t* src = a.dna + W.src;
	const int alen = W.alt_len < 0 ? W.ref_len : W.alt_len;
	for (int c = threadIdx.x; c < P.n; c += VT_THREADS) {
		const int j = (P.enc & 1) ? P.n - 1 - c : c;
		uint8_t letter;
		if (j < W.pre) letter = src[j];
		else if (j < W.pre + alen) letter = W.alt_len < 0 ? src[j] : a.alts[W.alt_off + (j - W.pre)];
		else letter = src[W.pre + W.ref_len + (j - W.pre - alen)];
		a.tcodes[P.tbase + c] = lut[letter];
	}
}

// One workgroup of NT threads per problem (NT = 64 or 128 for queries of at most that many rows, else 256).  Thread t owns rows
// [t * rpt, (t + 1) * rpt); the state of its i-th row lives at [i * NT + t], so that the lanes of a wave read and write neighbouring
// 16-bit words (no LDS bank conflicts, coalesced in HBM).
// IN_LDS: dynamic LDS of [lds_rows] x (3 x uint16 + 1 code byte), lds_rows = rpt * NT (every pointer of the column step is then an LDS
// pointer at compile time: ds_read_u16, not a flat load); otherwise the row state lives in a.rows and the codes are read from HBM
template <int NT, bool IN_LDS>
__global__ void __launch_bounds__(NT) k_touch(TouchLaunch a, int lds_rows)
{
	extern __shared__ __align__(16) unsigned char vt_lds[];
	__shared__ int wtot[4];
	__shared__ unsigned best_sh;
	const int p = blockIdx.x;
	if (p >= a.nprob) return;
	const TouchProb P = a.probs[p];
	const int m = a.m, t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int rpt = (m + NT - 1) / NT;
	const int first = min(m, t * rpt), cnt = min(m, first + rpt) - first;
	VtState S;
	if (IN_LDS) {
		uint16_t* b = reinterpret_cast<uint16_t*>(vt_lds);
		S.h[0] = b; S.h[1] = b + lds_rows; S.e = b + 2 * lds_rows;
		uint8_t* qc = reinterpret_cast<uint8_t*>(b + 3 * lds_rows);
		for (int i = 0; i < rpt; i++) qc[i * NT + t] = i < cnt ? a.qcodes[first + i] : 4;
		S.q = qc;
	} else {
		uint16_t* b = a.rows + (int64_t)p * 3 * rpt * NT;
		S.h[0] = b; S.h[1] = b + rpt * NT; S.e = b + 2 * rpt * NT;
		S.q = a.qcodes;
	}
	// Every thread walks rpt rows: the rows from m on (the last rows of the last threads) lie below every real row, so nothing of
	// them reaches a real cell; they are only kept out of the maximum.  The code of the thread's i-th row: S.q[q0 + i * qstep]
	const int qstep = IN_LDS ? NT : 1, q0 = IN_LDS ? t : min(first, m - 1), qlast = IN_LDS ? rpt - 1 : m - 1 - q0;
	const int above = (rpt - 1) * NT + t - 1;                                      // the last row of the thread before this one
	for (int i = 0; i < rpt; i++) { S.h[0][i * NT + t] = 0; S.e[i * NT + t] = 0; }
	if (t == 0) best_sh = 0;
	__syncthreads();
	const bool ok = P.n >= 1 && P.n <= TOUCH_MAX_COLS && P.v0 >= 0 && P.v0 < P.v1 && P.v1 <= P.n;      // (uniform)
	const uint8_t* tc = a.tcodes + P.tbase;
	int best = 0;
	for (int c = 0; ok && c < P.n; c++) {
		const uint16_t* cur = (c & 1) ? S.h[1] : S.h[0];
		uint16_t* nxt = (c & 1) ? S.h[0] : S.h[1];
		const int tcode = tc[c];
		const bool cont = c >= P.v1;                 // behind the allele the diagonal only continues an alignment
		const int mark = ((c == 0 && (P.edge & 1)) || (c == P.n - 1 && (P.edge & 2))) ? 1 : 0;
		const int top = t > 0 ? (int)cur[above] : 0;      // H of the previous column in the row above the thread's first
		// first walk: E, and H with the vertical gaps that open in the thread's own rows (hl); what these rows hand to the row below
		// them.  A gap never opens better from a cell that a gap reached (h - 32 < f - 8 where h = f), so the gap value of a row is
		// max(f - 8, h - 32) whichever h, the final one or hl, stands in it.
		const bool counts = c >= P.v0;
		int out;
		{
			int hd = top, f = 0, hn = 0;
			for (int i0 = 0; i0 < rpt; i0 += VT_UNROLL) {
				int hc[VT_UNROLL], ein[VT_UNROLL], sc[VT_UNROLL];
#pragma unroll
				for (int k = 0; k < VT_UNROLL; k++) {      // (the loads of a short last group repeat its last row: no branch around a load)
					const int i = min(i0 + k, rpt - 1);
					hc[k] = cur[i * NT + t]; ein[k] = S.e[i * NT + t]; sc[k] = vt_score2(S.q[q0 + min(i, qlast) * qstep], tcode);
				}
#pragma unroll
				for (int k = 0; k < VT_UNROLL; k++) if (i0 + k < rpt) {
					const int e = vt_floor(max(ein[k] - 8, hc[k] - 32));
					if (i0 + k > 0) f = vt_floor(max(f - 8, hn - 32));
					int dg = hd + sc[k];
					if (cont) dg = hd ? dg : 0;
					int h = max(vt_floor(max(dg, e)), f);
					if (mark && h) h |= 1;
					if (counts && i0 + k < cnt) best = max(best, h);
					nxt[(i0 + k) * NT + t] = (uint16_t)h; S.e[(i0 + k) * NT + t] = (uint16_t)e;
					hd = hc[k]; hn = h;
				}
			}
			out = max(f - 8, hn - 32);
		}
		const int ex = vt_scan_excl<NT>(out + 8 * rpt * t, wtot, lane, wave);
		const int fin = t == 0 ? 0 : vt_floor(max(ex, VT_NEG32) - 8 * rpt * (t - 1));
		// second walk, where a gap enters a thread of the wave from above: H = max(hl, the gap continued from fin)
		if (__any(fin > 0)) {
			int f = fin, hn = 0;
			for (int i = 0; i < rpt; i++) {
				if (i > 0) f = vt_floor(max(f - 8, hn - 32));
				const int h = max((int)nxt[i * NT + t], f);      // (f carries the bit of the marked cell it comes from)
				if (counts && i < cnt) best = max(best, h);
				nxt[i * NT + t] = (uint16_t)h;
				hn = h;
			}
		}
		__syncthreads();
	}
	if (best) atomicMax(&best_sh, (unsigned)best);      // (LDS)
	__syncthreads();
	if (t == 0) a.out[p] = best_sh;
}

__device__ __forceinline__ int vt_class(int enc) { return enc < 12 ? (enc & 1) : (((enc - 12) & 1) ? 3 : 2); }

// one thread per variant of the launch
__global__ void __launch_bounds__(VT_THREADS) k_touch_reduce(TouchReduceLaunch a)
{
	const int v = blockIdx.x * VT_THREADS + threadIdx.x;
	if (v >= a.nvar) return;
	unsigned top = 0;
	for (int al = 0; al < 2; al++) {
		const uint32_t* x = a.touch + ((int64_t)v * 2 + al) * a.nenc;
		for (int cls = 0; cls < 4; cls++) {
			unsigned bx = 0, be = 0xff;
			for (int k = 0; k < a.nenc; k++) {
				if (vt_class(a.enc[k]) != cls) continue;
				const unsigned w = x[k];
				if ((w >> 1) > (bx >> 1)) be = a.enc[k];      // (the encodings come in ascending order)
				bx = max(bx, w);
			}
			top = max(top, bx);
			a.out[(int64_t)v * 9 + al * 4 + cls] = (bx << 8) | be;
		}
	}
	a.out[(int64_t)v * 9 + 8] = top & 1;
}

static size_t vt_lds_bytes(int rows) { return (size_t)rows * 7 + 16; }

hipError_t launch_var_encode(const VarEncodeLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (!L.dna || !L.alts || !L.wins || !L.probs || !L.enc_lut || !L.tcodes) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_var_encode, dim3((unsigned)L.nprob), dim3(VT_THREADS), 0, st, L);
	return hipGetLastError();
}

int touch_threads(int m) { return m <= 64 ? 64 : (m <= 128 ? 128 : VT_THREADS); }
int touch_state_rows(int m) { const int nt = touch_threads(m); return (m + nt - 1) / nt * nt; }

hipError_t launch_touch(const TouchLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (L.m < 1 || !L.tcodes || !L.qcodes || !L.probs || !L.out) return hipErrorInvalidValue;
	const bool lds = L.m <= TOUCH_LDS_ROWS;
	if (!lds && !L.rows) return hipErrorInvalidValue;
	const int nt = touch_threads(L.m);
	const int lds_rows = lds ? touch_state_rows(L.m) : 0;
	const dim3 grid((unsigned)L.nprob);
	if (!lds) hipLaunchKernelGGL((k_touch<VT_THREADS, false>), grid, dim3(VT_THREADS), 0, st, L, 0);
	else if (nt == 64) hipLaunchKernelGGL((k_touch<64, true>), grid, dim3(64), vt_lds_bytes(lds_rows), st, L, lds_rows);
	else if (nt == 128) hipLaunchKernelGGL((k_touch<128, true>), grid, dim3(128), vt_lds_bytes(lds_rows), st, L, lds_rows);
	else hipLaunchKernelGGL((k_touch<VT_THREADS, true>), grid, dim3(VT_THREADS), vt_lds_bytes(lds_rows), st, L, lds_rows);
	return hipGetLastError();
}

hipError_t launch_touch_reduce(const TouchReduceLaunch& L, hipStream_t st)
{
	if (L.nvar <= 0) return hipSuccess;
	if (!L.touch || !L.out || L.nenc < 1 || L.nenc > 48) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_touch_reduce, dim3((unsigned)((L.nvar + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
