// fasim-longtarget_amd/csrc/scan_short.hip -- k_scan_short: the column maxima of a short oligo (1 .. 112 nt) against every unit of a
// batch, for gfx950.
//
// The values are those of section 11 -- plain Gotoh local alignment, +5 / -4 over ACGT, every other letter -4, first gap residue
// 16, each further one 4, floor 0, the oligo padded with zero-score rows to ROWS = 16 * ceil(m / 16) -- and the output is k_scan's:
// colmax16[unit][column] = 2 * maximum, taint bit 0, so k_track and k_sites take it as it is.  What differs is the shape of the work.
// An oligo has so few rows that a lane can hold the whole DP column, and an alignment that decides a column maximum starts at
// most W(m) = ROWS + max(0, (5 m - 13) div 4) columns before it (at most ROWS pairs, and DNA-side gap residues of cost 4 D + 12 < 5 m).
// So the columns of a unit are separable: a DP started from zeros W columns early is exact from the first wanted column on.
//
//   * a lane owns two stretches of L columns of one unit, one in each half of its packed registers: stretch 2 p in the low halves,
//     stretch 2 p + 1 in the high halves.  It starts `warm` columns early (W rounded up to 16; columns before the unit's first are
//     code N, under which the zero state stays zero) and stores nothing while it warms up;
//   * H and E of all ROWS rows stay in VGPRs as packed f16 (dp_f16.h: every value is an integer of magnitude <= 1 024 here, since a score
//     is at most 5 * 112 = 560, so f16 sums and maxima are the integers themselves).  One row of one column pair is
//         t = Hdiag + s ; h = max3(t, E, F) ; ho = h - 16 ; E = max3(E - 4, ho, 0) ; F = max3(F - 4, ho, 0)
//     and half a max3 for the column maximum: 7.5 packed instructions.  No taint, no saturation, no overflow flag;
//   * the oligo is uniform over the launch: the workgroup first builds prof[row][5 * code_lo + code_hi] = the packed score pair of
//     that row in LDS (ROWS x 25 dwords).  A row's score is then one ds_read_b32 whose address is the column pair's own and whose
//     row offset is an immediate -- the lanes of a wave read at most 25 neighbouring dwords, so there is no bank conflict;
//   * target codes arrive as one aligned 16-byte load per stretch and 16 columns, column maxima leave as one aligned 8-byte store
//     per stretch and 4 columns: a lane's accesses walk its own cache lines, 16 (or 8) bytes at a time.  Columns from the
//     unit's length up to the next multiple of 16 are stored as 0, the ones behind them not at all.
//
// No scratch, no atomics, no work queue: one lane per stretch pair, grid = units x pairs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "kernels.h"
#include "dp_f16.h"

namespace fasim {

int scan_short_warmup(int m)
{
	const int rows = 16 * ((m + 15) / 16);
	return rows + std::max(0, (5 * m - 13) / 4);
}

namespace {

constexpr uint32_t SS_N4 = 0x04040404u;          // four columns of code N
constexpr uint32_t SS_F16_NEG4 = 0xC400u;        // f16 -4.0

__device__ __forceinline__ uint32_t ss_add(uint32_t a, uint32_t b) { uint32_t r; asm("v_pk_add_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
typedef unsigned short ss_v2us __attribute__((ext_vector_type(2)));
// v_pk_max_u16 (a builtin, not an asm: the accumulators may then stay in AGPRs between their uses)
__device__ __forceinline__ uint32_t ss_umax(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(ss_v2us, a), __builtin_bit_cast(ss_v2us, b)));
}

template <int ROWS>
__global__ void __launch_bounds__(256) k_scan_short(ScanShortLaunch a)
{
	__shared__ uint32_t prof[ROWS * 25];
	for (int idx = threadIdx.x; idx < ROWS * 25; idx += 256) {
		const int row = idx / 25, combo = idx - row * 25, clo = combo / 5, chi = combo - clo * 5;
		uint32_t lo = 0, hi = 0;                 // pad rows score 0
		if (row < a.m) {
			const int q = a.qcodes[row];
			lo = (q == clo && q < 4) ? f16c(5) : SS_F16_NEG4;
			hi = (q == chi && q < 4) ? f16c(5) : SS_F16_NEG4;
		}
		prof[idx] = lo | (hi << 16);
	}
	__syncthreads();

	const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const int unit = (int)(item / a.npairs), pair = (int)(item - (int64_t)unit * a.npairs);
	if (unit >= a.nunit) return;
	const int n = a.unit_len[unit], n16 = min((n + 15) & ~15, a.tstride), L = a.stretch, tstride = a.tstride;
	const int sA = 2 * pair * L, sB = sA + L;     // first columns of the two stretches
	if (sA >= n) return;
	const uint8_t* trow = a.tcodes + (int64_t)unit * tstride;
	uint16_t* orow = a.colmax16 + (int64_t)unit * tstride;
	const uint32_t k4 = f16c2(4), k16 = f16c2(16), k1024 = f16c2(1024);

	uint32_t H[ROWS], E[ROWS];
#pragma unroll
	for (int i = 0; i < ROWS; i++) { H[i] = 0; E[i] = 0; }

#pragma unroll 1
	for (int g = -a.warm; g < L; g += 16) {
		const int cA = sA + g, cB = sB + g;       // multiples of 16, like tstride: a group lies inside the unit's row or outside it
		uint4 wa = make_uint4(SS_N4, SS_N4, SS_N4, SS_N4), wb = wa;
		if (cA >= 0 && cA < tstride) wa = *reinterpret_cast<const uint4*>(trow + cA);
		if (cB >= 0 && cB < tstride) wb = *reinterpret_cast<const uint4*>(trow + cB);
#pragma unroll 1
		for (int q4 = 0; q4 < 4; q4++) {
			uint32_t xa = wa.x, xb = wb.x;
			uint32_t oa0 = 0, oa1 = 0, ob0 = 0, ob1 = 0;
			const int ca = cA + 4 * q4, cb = cB + 4 * q4;
#pragma unroll 1
			for (int k = 0; k < 4; k++) {
				const uint32_t* pr = prof + (min(xa & 0xffu, 4u) * 5u + min(xb & 0xffu, 4u));
				xa >>= 8; xb >>= 8;
				uint32_t diag = 0, f = 0, cm = 0;
#pragma unroll
				for (int i = 0; i < ROWS; i += 2) {
					const uint32_t t0 = ss_add(diag, pr[i * 25]);
					const uint32_t t1 = ss_add(H[i], pr[(i + 1) * 25]);
					diag = H[i + 1];
					const uint32_t h0 = (uint32_t)hf_max3((int)t0, (int)E[i], (int)f);
					const uint32_t ho0 = (uint32_t)hf_sub_k((int)h0, k16);
					E[i] = (uint32_t)hf_max_floor(hf_sub_k((int)E[i], k4), (int)ho0);
					f = (uint32_t)hf_max_floor(hf_sub_k((int)f, k4), (int)ho0);
					H[i] = h0;
					const uint32_t h1 = (uint32_t)hf_max3((int)t1, (int)E[i + 1], (int)f);
					const uint32_t ho1 = (uint32_t)hf_sub_k((int)h1, k16);
					E[i + 1] = (uint32_t)hf_max_floor(hf_sub_k((int)E[i + 1], k4), (int)ho1);
					f = (uint32_t)hf_max_floor(hf_sub_k((int)f, k4), (int)ho1);
					H[i + 1] = h1;
					cm = (uint32_t)hf_max3((int)cm, (int)h0, (int)h1);
				}
				// M < 1 024: the f16 bits of M + 1 024 are 0x6400 + M
				uint32_t x = (ss_add(cm, k1024) & 0x03ff03ffu) << 1;
				if (ca + k >= n) x &= 0xffff0000u;
				if (cb + k >= n) x &= 0x0000ffffu;
				oa0 = __builtin_amdgcn_alignbit(oa1, oa0, 16); oa1 = (oa1 >> 16) | (x << 16);
				ob0 = __builtin_amdgcn_alignbit(ob1, ob0, 16); ob1 = (ob1 >> 16) | (x & 0xffff0000u);
			}
			if (g >= 0) {
				if (ca < n16) *reinterpret_cast<uint2*>(orow + ca) = make_uint2(oa0, oa1);
				if (cb < n16) *reinterpret_cast<uint2*>(orow + cb) = make_uint2(ob0, ob1);
			}
			wa = make_uint4(wa.y, wa.z, wa.w, wa.x); wb = make_uint4(wb.y, wb.z, wb.w, wb.x);
		}
	}
}

// ---- k_scan_short_rows: the same pass, which also leaves the row maxima of the lane's two stretches ------------
// One more packed accumulator per row, R[i] = v_pk_max_u16(R[i], H[i] & mk) on the f16 bit patterns: the values are non-negative
// integers, so the bits order like the values.  mk is the validity mask of the column pair: only the REAL columns of the lane's own
// stretches count, g >= 0 and column < n.  A column of code N behind the unit's last continues the diagonal at -4 per step and can
// exceed everything its row really holds; a warm-up column is a real column of the neighbouring stretch, or code N ahead of the unit,
// and holds a lower bound of what the neighbour computes there, so leaving it out changes nothing.  One body for all groups: choosing
// among an unmasked and a masked body per group costs the compiler the registers (section 24 has the numbers).
// At its end the lane folds the two halves and writes rowpart16[unit][pair][ROWS] = 2 * value with plain 16-byte stores.  A lane that
// returns early writes nothing: the fold (k_rowfold_parts, rowfold.hip) skips the parts with 2 * pair * L >= n.
template <int ROWS>
__global__ void __launch_bounds__(256) k_scan_short_rows(ScanShortLaunch a)
{
	__shared__ uint32_t prof[ROWS * 25];
	for (int idx = threadIdx.x; idx < ROWS * 25; idx += 256) {
		const int row = idx / 25, combo = idx - row * 25, clo = combo / 5, chi = combo - clo * 5;
		uint32_t lo = 0, hi = 0;                 // pad rows score 0
		if (row < a.m) {
			const int q = a.qcodes[row];
			lo = (q == clo && q < 4) ? f16c(5) : SS_F16_NEG4;
			hi = (q == chi && q < 4) ? f16c(5) : SS_F16_NEG4;
		}
		prof[idx] = lo | (hi << 16);
	}
	__syncthreads();

	const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const int unit = (int)(item / a.npairs), pair = (int)(item - (int64_t)unit * a.npairs);
	if (unit >= a.nunit) return;
	const int n = a.unit_len[unit], n16 = min((n + 15) & ~15, a.tstride), L = a.stretch, tstride = a.tstride;
	const int sA = 2 * pair * L, sB = sA + L;     // first columns of the two stretches
	if (sA >= n) return;
	const uint8_t* trow = a.tcodes + (int64_t)unit * tstride;
	uint16_t* orow = a.colmax16 + (int64_t)unit * tstride;
	const uint32_t k4 = f16c2(4), k16 = f16c2(16), k1024 = f16c2(1024);

	uint32_t H[ROWS], E[ROWS], R[ROWS];
#pragma unroll
	for (int i = 0; i < ROWS; i++) { H[i] = 0; E[i] = 0; R[i] = 0; }

#pragma unroll 1
	for (int g = -a.warm; g < L; g += 16) {
		const int cA = sA + g, cB = sB + g;       // multiples of 16, like tstride: a group lies inside the unit's row or outside it
		uint4 wa = make_uint4(SS_N4, SS_N4, SS_N4, SS_N4), wb = wa;
		if (cA >= 0 && cA < tstride) wa = *reinterpret_cast<const uint4*>(trow + cA);
		if (cB >= 0 && cB < tstride) wb = *reinterpret_cast<const uint4*>(trow + cB);
		const int nv = g >= 0 ? n : 0;            // columns below nv count for the row maxima
#pragma unroll 1
		for (int q4 = 0; q4 < 4; q4++) {
			uint32_t xa = wa.x, xb = wb.x;
			uint32_t oa0 = 0, oa1 = 0, ob0 = 0, ob1 = 0;
			const int ca = cA + 4 * q4, cb = cB + 4 * q4;
#pragma unroll 1
			for (int k = 0; k < 4; k++) {
				const uint32_t* pr = prof + (min(xa & 0xffu, 4u) * 5u + min(xb & 0xffu, 4u));
				xa >>= 8; xb >>= 8;
				const uint32_t mk = (ca + k < nv ? 0x0000ffffu : 0u) | (cb + k < nv ? 0xffff0000u : 0u);
				uint32_t diag = 0, f = 0, cm = 0;
#pragma unroll
				for (int i = 0; i < ROWS; i += 2) {
					const uint32_t t0 = ss_add(diag, pr[i * 25]);
					const uint32_t t1 = ss_add(H[i], pr[(i + 1) * 25]);
					diag = H[i + 1];
					const uint32_t h0 = (uint32_t)hf_max3((int)t0, (int)E[i], (int)f);
					const uint32_t ho0 = (uint32_t)hf_sub_k((int)h0, k16);
					E[i] = (uint32_t)hf_max_floor(hf_sub_k((int)E[i], k4), (int)ho0);
					f = (uint32_t)hf_max_floor(hf_sub_k((int)f, k4), (int)ho0);
					H[i] = h0;
					R[i] = ss_umax(R[i], h0 & mk);
					const uint32_t h1 = (uint32_t)hf_max3((int)t1, (int)E[i + 1], (int)f);
					const uint32_t ho1 = (uint32_t)hf_sub_k((int)h1, k16);
					E[i + 1] = (uint32_t)hf_max_floor(hf_sub_k((int)E[i + 1], k4), (int)ho1);
					f = (uint32_t)hf_max_floor(hf_sub_k((int)f, k4), (int)ho1);
					H[i + 1] = h1;
					R[i + 1] = ss_umax(R[i + 1], h1 & mk);
					cm = (uint32_t)hf_max3((int)cm, (int)h0, (int)h1);
				}
				// M < 1 024: the f16 bits of M + 1 024 are 0x6400 + M
				uint32_t x = (ss_add(cm, k1024) & 0x03ff03ffu) << 1;
				if (ca + k >= n) x &= 0xffff0000u;
				if (cb + k >= n) x &= 0x0000ffffu;
				oa0 = __builtin_amdgcn_alignbit(oa1, oa0, 16); oa1 = (oa1 >> 16) | (x << 16);
				ob0 = __builtin_amdgcn_alignbit(ob1, ob0, 16); ob1 = (ob1 >> 16) | (x & 0xffff0000u);
			}
			if (g >= 0) {
				if (ca < n16) *reinterpret_cast<uint2*>(orow + ca) = make_uint2(oa0, oa1);
				if (cb < n16) *reinterpret_cast<uint2*>(orow + cb) = make_uint2(ob0, ob1);
			}
			wa = make_uint4(wa.y, wa.z, wa.w, wa.x); wb = make_uint4(wb.y, wb.z, wb.w, wb.x);
		}
	}

	// the two stretches of a lane belong to one unit: the larger half, as 2 * value, eight rows per store
	uint16_t* prow = a.rowpart16 + item * ROWS;
#pragma unroll
	for (int i = 0; i < ROWS; i += 8) {
		uint32_t w[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t x0 = ss_add(R[i + 2 * j], k1024) & 0x03ff03ffu, x1 = ss_add(R[i + 2 * j + 1], k1024) & 0x03ff03ffu;
			w[j] = (max(x0 & 0xffffu, x0 >> 16) << 1) | (max(x1 & 0xffffu, x1 >> 16) << 17);
		}
		*reinterpret_cast<uint4*>(prow + i) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

template <int ROWS>
hipError_t ss_launch(const ScanShortLaunch& L, hipStream_t st)
{
	const int64_t items = (int64_t)L.nunit * L.npairs;
	if (L.rowpart16) hipLaunchKernelGGL(k_scan_short_rows<ROWS>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, L);
	else hipLaunchKernelGGL(k_scan_short<ROWS>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, L);
	return hipGetLastError();
}

} // namespace

void scan_short_shape(int m, int tstride, int nunit, int* stretch, int* npairs, int* warm)
{
	const int w = (scan_short_warmup(m) + 15) & ~15;
	// stretches of at least four warm-ups (256 columns at the least) keep the warm-up below a fifth of the work; within that, as
	// many stretch pairs per unit as it takes to give the launch 256 waves (the workers keep several launches in flight), and at
	// least one per 2 560 columns
	const int least = std::max(1, (tstride + 2559) / 2560), most = std::max(least, tstride / (2 * std::max(256, 4 * w)));
	const int np = (int)std::min<int64_t>(most, std::max<int64_t>(least, (256 * 64 + (int64_t)nunit - 1) / std::max(1, nunit)));
	int len = ((tstride + 2 * np - 1) / (2 * np) + 15) & ~15;
	len = std::max(len, w);
	*stretch = len; *npairs = (tstride + 2 * len - 1) / (2 * len); *warm = w;
}

hipError_t launch_scan_short(const ScanShortLaunch& L, hipStream_t st)
{
	if (L.nunit <= 0) return hipSuccess;
	if (L.m < 1 || L.m > SCAN_SHORT_MAX || L.stretch < 16 || (L.stretch & 15) || (L.warm & 15) || (L.tstride & 15) || L.npairs < 1 ||
		L.warm < scan_short_warmup(L.m) || (int64_t)2 * L.npairs * L.stretch < L.tstride) return hipErrorInvalidValue;
	switch ((L.m + 15) / 16) {
	case 1: return ss_launch<16>(L, st);
	case 2: return ss_launch<32>(L, st);
	case 3: return ss_launch<48>(L, st);
	case 4: return ss_launch<64>(L, st);
	case 5: return ss_launch<80>(L, st);
	case 6: return ss_launch<96>(L, st);
	default: return ss_launch<112>(L, st);
	}
}

} // namespace fasim
