// fasim-longtarget_amd/csrc/systolic.h -- the systolic wave pipeline shared by k_scan (scan.hip), k_align_fwd (align.hip) and
// k_align_band (band.hip) for gfx950: one text for the vocabulary, the geometry, the LDS profile, the Gotoh row pair and the
// Q2 row analysis.
//
// The pipeline: 128 virtual lanes = 64 lanes x 2 packed 16-bit halves.  Virtual lane v owns RP consecutive query rows (H and E
// of those rows live in VGPRs as packed u16 pairs) and works on column (step - v) at pipeline step `step`, so every dependency
// (diagonal H, vertical F, running maxima, target code) arrives from virtual lane v - 1 one step earlier: one DPP move and one
// v_alignbit each.  All cell arithmetic is packed 16-bit VALU, two DP cells per instruction.
//
// What a kernel gets from this header:
//   * vocabulary: v2s / v2u / v4i and their bit casts; the packed helpers that must stay inline asm (each says why); the hand-over
//     shift vshift / vshift0 / vprev0 with the DPP control and the start-lane fix-up as template parameters;
//   * geometry: lane_rows (the stripe-aligned row layout: each of the reference's 16 stripes is exactly `vs` virtual lanes, so the
//     F entering virtual lane vs * k IS the F crossing stripe boundary k), the LDS profile layout PROF_*, and StripeLane, the
//     per-lane constants of that layout;
//   * profile: stage_profile writes prof[code][lane][half][row] from a score functor; ProfileRows<RP> fetches the rows of a lane's
//     two codes with ds_read_b128 and merges them per row with one v_perm_b32 (score_of);
//   * the row pair: int_row_pair and f16_row_pair (k_scan, k_align_fwd) compute one column of RP rows for both halves.  They guarantee that the new H
//     column is written into the registers of the old one (tied operands: no column copy at the end of a step), that every
//     diagonal sum goes into the register of its score, and that the lane maximum runs in independent chains;
//   * q2_rows: the Q2 row analysis, once, for any value scale.  It reads H / E in a first pass and modifies
//     them in place in a second, so the registers of the common path cross the rare branch without copies.
// What a kernel must still do itself: own its LDS (the profile buffer and anything next to it), its work loop and its step loop,
// its hand-over sources (zeros, the previous tile's bottom row, a feeder), its pipe end, and its barriers: stage_profile does
// not synchronise, the caller puts __syncthreads() between staging and the first ProfileRows.
// k_align_band takes everything but int_row_pair: its row loop is written out in band.hip on h_in_place / diag_plus_score,
// because through int_row_pair the compiler schedules its 4-step loop differently (profiles/r17_systolic_isa.txt).
// Everything here is __device__ __forceinline__ or constexpr.  Against the kernels' own copies the step loops keep the packed,
// LDS-read and DPP counts and the VALU count of the common path; what moves is scalar code and s_nop padding, the latter in
// the rare Q2 blocks (same file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"
#include "dp_f16.h"

namespace fasim {

// ---- vocabulary -----------------------------------------------------------------------------------
// H and E are kept as plain 32-bit registers (two packed u16 halves each) and only viewed as vectors inside the arithmetic:
// vector-typed loop-carried values get split into halves and re-packed by the compiler
typedef short v2s __attribute__((ext_vector_type(2)));
typedef unsigned short v2u __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v2s as_s(v2u x) { return __builtin_bit_cast(v2s, x); }
__device__ __forceinline__ v2u as_u(v2s x) { return __builtin_bit_cast(v2u, x); }
__device__ __forceinline__ v2s s_from(int x) { return __builtin_bit_cast(v2s, x); }
__device__ __forceinline__ v2u u_from(int x) { return __builtin_bit_cast(v2u, x); }
__device__ __forceinline__ int to_int(v2s x) { return __builtin_bit_cast(int, x); }
__device__ __forceinline__ int to_int(v2u x) { return __builtin_bit_cast(int, x); }

// Packed 16-bit helpers for the (rare) hazard branch, written as inline asm so that the compiler neither rewrites
// them into per-half compares/selects nor hoists them into the main path of every step.
__device__ __forceinline__ v2u pk_subs(v2u a, v2u b) { v2u r; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ v2u pk_subs_k(v2u a, uint32_t k) { v2u r; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "s"(k)); return r; }
__device__ __forceinline__ v2u pk_ksubs(uint32_t k, v2u a) { v2u r; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "s"(k), "v"(a)); return r; }
__device__ __forceinline__ v2u pk_minu(v2u a, v2u b) { v2u r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ v2u pk_minu_k(v2u a, uint32_t k) { v2u r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "s"(k)); return r; }
__device__ __forceinline__ v2u pk_maxu(v2u a, v2u b) { v2u r; asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// x |= bits with input and output tied to ONE register: a value that the rare branch may modify then needs no copy at
// the join with the common path (plain C would let the allocator put the two versions into different registers and
// pay a v_mov per row in every step)
__device__ __forceinline__ void or_in_place(int& x, int bits) { asm volatile("v_or_b32 %0, %0, %1" : "+v"(x) : "v"(bits)); }
// acc = max(acc, x) on packed u16 with input and output tied to ONE register (as or_in_place: the running row maxima of k_scan's
// ROWS variant cross the rare hazard branch and two copies of the step body, and must not be copied at any join)
__device__ __forceinline__ void rowmax_in_place(int& acc, int x) { asm("v_pk_max_u16 %0, %0, %1" : "+v"(acc) : "v"(x)); }
// a packed pair of f16 integers -> the packed pair of u16 integers (inline asm: used in rare branches only, see pk_subs; volatile:
// the conversions of a whole H / E column must stay where they are written, one at a time, or their results all live at once
// and the register allocator spills in the common path)
__device__ __forceinline__ int hf_to_u16(int x)
{
	int r;
	asm volatile("v_cvt_u16_f16_e32 %0, %1\n\tv_cvt_u16_f16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\ts_nop 0" : "=&v"(r) : "v"(x));
	return r;
}

// The hand-over from virtual lane v - 1.  CTRL is the DPP control: wave_shr:1 for one pipeline per wave, row_shr:1 for the
// sub-pipelines of k_align_band.  FIX: the first lane of a (sub-)pipeline is not the first lane DPP leaves alone, so it is
// fixed up with `is_start` (a row_shr pipeline of exactly one row, and a wave_shr pipeline of the whole wave, need none).
constexpr int DPP_WAVE_SHR1 = 0x138, DPP_ROW_SHR1 = 0x111;
// x of lane - 1; the start lane gets `inject`
template <int CTRL = DPP_WAVE_SHR1, bool FIX = false>
__device__ __forceinline__ int vprev(int x, int inject, bool is_start = false)
{
	const int up = __builtin_amdgcn_update_dpp(inject, x, CTRL, 0xf, 0xf, false);
	return FIX ? (is_start ? inject : up) : up;
}
// the same with zeros entering the start lane (bound_ctrl: an out-of-range source lane reads as 0): no register has to be
// preloaded with the value to inject
template <int CTRL = DPP_WAVE_SHR1, bool FIX = false>
__device__ __forceinline__ int vprev0(int x, bool is_start = false)
{
	const int up = __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true);
	return FIX ? (is_start ? 0 : up) : up;
}
// shift a packed pair down the virtual-lane pipeline: out.lo = x.hi of lane - 1 (start lane: inject's hi half), out.hi = x.lo
template <int CTRL = DPP_WAVE_SHR1, bool FIX = false>
__device__ __forceinline__ int vshift(int x, int inject_hi, bool is_start = false) { return __builtin_amdgcn_alignbit(x, vprev<CTRL, FIX>(x, inject_hi, is_start), 16); }
template <int CTRL = DPP_WAVE_SHR1, bool FIX = false>
__device__ __forceinline__ int vshift0(int x, bool is_start = false) { return __builtin_amdgcn_alignbit(x, vprev0<CTRL, FIX>(x, is_start), 16); }

// ---- geometry -------------------------------------------------------------------------------------
// rows owned by global virtual lane v (stripe-aligned layout): stripe s = v / vs gets its ceil(m/16) rows spread over
// vs virtual lanes, the first (segLen % vs) of them one row longer
__device__ __forceinline__ void lane_rows(int v, int seg_len, int vs, int* row0, int* rows)
{
	const int s = v / vs, j = v - s * vs, q = seg_len / vs, rem = seg_len - q * vs;
	*rows = q + (j < rem ? 1 : 0);
	*row0 = s * seg_len + j * q + (j < rem ? j : rem);
}

// the LDS profile: int16 scores [code][lane][half][PROF_RS rows]; with the 112-byte lane stride the ds_read_b128 fetches (8 rows
// each) are bank-conflict free
constexpr int PROF_RS = 24;                           // storage rows per virtual lane
constexpr int PROF_HALF = 2 * PROF_RS;                // bytes from a lane's lo half to its hi half
constexpr int PROF_LANE_STRIDE = 112;                 // bytes: 2 halves x 24 rows x 2 B + 16 B pad
constexpr int PROF_CODE_STRIDE = 64 * PROF_LANE_STRIDE;   // 7168 B, a multiple of the 256-B bank row
constexpr int PROF_DEAD_F16 = -4096;                  // dead / void score of the f16 variants, whose values stay below 2048 (far from -inf: nothing may produce inf or NaN)

// per-lane constants of the stripe-aligned layout for the lane whose lo half is global virtual lane v0 (hi half: v0 + 1)
//   act / actm : 0xFFFF where the half owns RP rows, 0 where it owns RP - 1 (its last register row is transparent)
//   startm     : 0xFFFF where the half starts a stripe (v = vs * k, k >= 1): it sees F[b] of the boundary row b directly as its
//                incoming F and takes it as the start of a propagation chain
//   fthr2      : `thr` (F[b] >= 132 in the kernel's scale, minus one) in the stripe-start halves, 0xFFFF elsewhere: other halves never flag
//   row0       : first query row of each half
struct StripeLane {
	uint32_t act;
	v2u actm, startm, fthr2;
	int row0[2];
	__device__ __forceinline__ StripeLane(int v0, int seg_len, int vs, int rp, uint32_t thr)
	{
		uint32_t fthr = 0xFFFFFFFFu, startbits = 0;
		act = 0;
		for (int h = 0; h < 2; h++) {
			const int v = v0 + h;
			int rows_v;
			lane_rows(v, seg_len, vs, &row0[h], &rows_v);
			if (v % vs == 0 && v > 0) { fthr = (fthr & ~(0xFFFFu << (16 * h))) | (thr << (16 * h)); startbits |= 0xFFFFu << (16 * h); }
			if (rows_v == rp) act |= 0xFFFFu << (16 * h);
		}
		// (act is a plain register from here on: where the compiler can trace it back to the two compares, it turns the masks of the
		//  last register row into per-half selects)
		asm("" : "+v"(act));
		fthr2 = u_from((int)fthr);
		actm = u_from((int)act);
		startm = u_from((int)startbits);
	}
};

// ---- profile --------------------------------------------------------------------------------------
// stage prof[t][lane][half][r] for the 128 virtual lanes of query tile `tile`: score(t, global virtual lane, row in lane) -> int16.
// F16: the scores are stored as f16 bits, the dead score DEAD re-coded to PROF_DEAD_F16.  No barrier: the caller synchronises.
template <bool F16, int DEAD, class Score>
__device__ __forceinline__ void stage_profile(uint8_t* prof, int ncodes, int tile, Score score)
{
	for (int idx = threadIdx.x; idx < ncodes * 128 * PROF_RS; idx += blockDim.x) {
		const int r = idx % PROF_RS;
		const int v = (idx / PROF_RS) % 128;
		const int t = idx / (PROF_RS * 128);
		int sc = score(t, 128 * tile + v, r);
		if (F16) sc = (int)(int16_t)f16_bits(sc == DEAD ? PROF_DEAD_F16 : sc);
		*reinterpret_cast<int16_t*>(prof + t * PROF_CODE_STRIDE + (v >> 1) * PROF_LANE_STRIDE + (v & 1) * PROF_HALF + r * 2) = (int16_t)sc;
	}
}

// the profile rows of a lane's two codes: pa = the lo half's rows, pb = the hi half's (each RP int16, 16-byte aligned).  The two
// halves of a lane sit on different columns, so each fetches its own code's rows and a v_perm_b32 per row merges them.
template <int RP>
struct ProfileRows {
	static constexpr int ROWS_PER_LOAD = 8;
	static constexpr int NLOAD = (RP + ROWS_PER_LOAD - 1) / ROWS_PER_LOAD;
	v4i PA[NLOAD], PB[NLOAD];
	__device__ __forceinline__ ProfileRows(const uint8_t* pa, const uint8_t* pb)
	{
#pragma unroll
		for (int g = 0; g < NLOAD; g++) {
			PA[g] = *reinterpret_cast<const v4i*>(pa + 16 * g);
			PB[g] = *reinterpret_cast<const v4i*>(pb + 16 * g);
		}
	}
	__device__ __forceinline__ int score_of(int r) const
	{
		const int g = r / ROWS_PER_LOAD, k = r % ROWS_PER_LOAD;
		return __builtin_amdgcn_perm(PB[g][k >> 1], PA[g][k >> 1], (k & 1) ? 0x07060302 : 0x05040100);
	}
};

// ---- the row pair ---------------------------------------------------------------------------------
// CLAMP   : the diagonal sum saturates (values that may come near the end of the 16-bit range)
// ROW_TAG : the lane maximum is of h | (31 - r) (values scaled by >= 32: the maximum AND the smallest row that holds it); else of h
template <bool CLAMP_, bool ROW_TAG_>
struct IntRowPolicy { static constexpr bool CLAMP = CLAMP_, ROW_TAG = ROW_TAG_; };

// Row r needs the OLD H[r-1] (diagonal) and writes the NEW H[r].  The add of row r+1 (old H[r] + its score) is
// issued before H[r] is overwritten, so the new value can go into the same register: no second copy of the H
// column and no register moves at the end of the step.
// (the sum is forced into the register of the score, which dies there: the compiler would otherwise add in place
//  over the old H, keep that register busy until the next row and have to park the new H somewhere else)
template <bool CLAMP>
__device__ __forceinline__ v2s diag_plus_score(int hold, int sc)
{
	if (CLAMP) asm("v_pk_add_i16 %0, %1, %0 clamp" : "+v"(sc) : "v"(hold));
	else asm("v_pk_add_i16 %0, %1, %0" : "+v"(sc) : "v"(hold));
	return s_from(sc);
}

// max(h, f), written into the register that held the OLD H[r] (tied dummy operand `hold`; its last real use was the sum for row
// r+1): the H column stays where it is from step to step.  `after` (that sum) is an unused operand that only orders this behind
// it, because it still reads the old H[r].
__device__ __forceinline__ int h_in_place(int hold, int h, int f, int after)
{
	int hn;
	asm("v_pk_max_i16 %0, %2, %3" : "=v"(hn) : "0"(hold), "v"(h), "v"(f), "v"(after));
	return hn;
}

// One column of the integer Gotoh recurrence over the RP rows of both halves.  In: hdiag0 = H[row0 - 1] of the previous column,
// f = the F entering the first row; gapo / dec = gap open / extension in the kernel's scale (constants, or per-lane registers that
// hold 0xFFFF in void columns); the last register row is masked by `act` (a half owns RP or RP - 1 rows).  Out: H, E, f (leaving the last owned row), hbot (H of the last owned row); returns the lane maximum.
// row_hook(r, h) runs after H[r] is written; top_hook(r, t) before row r's maximum (k_scan's DUMP: the second E / restarted-F chain).
template <class P, int RP, class Prof, class RowHook, class TopHook>
__device__ __forceinline__ v2s int_row_pair(int (&H)[RP], int (&E)[RP], int& hbot, v2u& f, int hdiag0, const Prof& prof, v2u gapo, v2u dec,
	uint32_t act, RowHook row_hook, TopHook top_hook)
{
	const v2u actm = u_from((int)act);
	v2s lmx[4] = { (v2s){ 0, 0 }, (v2s){ 0, 0 }, (v2s){ 0, 0 }, (v2s){ 0, 0 } };   // independent chains: no back-to-back dependent v_pk_max
	v2s t = diag_plus_score<P::CLAMP>(hdiag0, prof.score_of(0));
#pragma unroll
	for (int r = 0; r < RP; r++) {
		v2s tnext = t;
		if (r + 1 < RP) tnext = diag_plus_score<P::CLAMP>(H[r], prof.score_of(r + 1));
		top_hook(r, t);
		v2s h = __builtin_elementwise_max(t, s_from(E[r]));
		h = s_from(h_in_place(H[r], to_int(h), to_int(f), to_int(tnext)));
		H[r] = to_int(h);
		row_hook(r, to_int(h));
		const v2u ho = __builtin_elementwise_sub_sat(as_u(h), gapo);
		E[r] = to_int(__builtin_elementwise_max(__builtin_elementwise_sub_sat(u_from(E[r]), dec), ho));
		const v2u fnew = __builtin_elementwise_max(__builtin_elementwise_sub_sat(f, dec), ho);
		const v2s key = P::ROW_TAG ? (h | (v2s){ (short)(31 - r), (short)(31 - r) }) : h;
		if (r == RP - 1) {
			// a half that owns only RP-1 rows passes F and its bottom H through unchanged
			f = (fnew & actm) | (f & ~actm);
			const int hm = to_int(h) & (int)act;        // (without row tags this is also what the lane maximum sees: one AND for both)
			lmx[r & 3] = __builtin_elementwise_max(lmx[r & 3], P::ROW_TAG ? as_s(as_u(key) & actm) : s_from(hm));
			if (RP > 1) hbot = hm | (H[RP > 1 ? RP - 2 : 0] & ~(int)act);
			else hbot = to_int(h);
		} else {
			f = fnew;
			lmx[r & 3] = __builtin_elementwise_max(lmx[r & 3], key);
		}
		t = tnext;
	}
	return __builtin_elementwise_max(__builtin_elementwise_max(lmx[0], lmx[1]), __builtin_elementwise_max(lmx[2], lmx[3]));
}

// gap operands of the f16 row pair: packed f16 constants in scalar registers, or per-lane registers (+inf in void columns)
template <uint32_t KOPEN, uint32_t KEXT>
struct HfGapConst {
	__device__ __forceinline__ int open(int h) const { return hf_sub_k(h, KOPEN); }
	__device__ __forceinline__ int ext(int x) const { return hf_sub_k(x, KEXT); }
};
struct HfGapReg {
	int gapo, dec;
	__device__ __forceinline__ int open(int h) const { return hf_sub(h, gapo); }
	__device__ __forceinline__ int ext(int x) const { return hf_sub(x, dec); }
};

// The same column in packed f16 (dp_f16.h): 8.5 instructions per row pair where the integer one takes 10.  The last register row
// is always masked by `act`.  ff: F in and out; returns the lane maximum (f16 bits; non-negative, so they order like the values).
template <int RP, class Prof, class Gap, class RowHook>
__device__ __forceinline__ int f16_row_pair(int (&H)[RP], int (&E)[RP], int& hbot, int& ff, int hdiag0, const Prof& prof, const Gap& gap,
	uint32_t act, RowHook row_hook)
{
	int lm0 = 0, lm1 = 0, hprev = 0;
	int t = hf_diag_plus_score(hdiag0, prof.score_of(0));
#pragma unroll
	for (int r = 0; r < RP; r++) {
		int tnext = t;
		if (r + 1 < RP) tnext = hf_diag_plus_score(H[r], prof.score_of(r + 1));
		const int h = hf_h(H[r], t, E[r], ff, tnext);
		H[r] = h;
		row_hook(r, h);
		const int ho = gap.open(h);
		E[r] = hf_max_floor(gap.ext(E[r]), ho);
		const int fnew = hf_max_floor(gap.ext(ff), ho);
		int hm = h;             // what the lane maximum sees of this row
		if (r == RP - 1) {
			ff = (fnew & (int)act) | (ff & ~(int)act);
			hm = h & (int)act;
			if (RP > 1) hbot = hm | (H[RP > 1 ? RP - 2 : 0] & ~(int)act);
			else hbot = h;
		} else ff = fnew;
		// one max3 per two rows, two independent chains
		if (r & 1) { if (r & 2) lm1 = hf_max3(lm1, hprev, hm); else lm0 = hf_max3(lm0, hprev, hm); }
		hprev = hm;
		t = tnext;
	}
	return (RP & 1) ? hf_max3(lm0, lm1, hprev) : hf_max_floor(lm0, lm1);
}

// ---- Q2 row analysis ------------------------------------------------------------------------------
// The reference's lazy-F loop leaves early (signed compare, sswNew.cpp:369) only while a stripe's propagated boundary value
// Fp = F[b] - 4j is >= 132 and the H it has just corrected is < 144 (then vF >= 128 reads as negative, vH < 128 as positive).
// From then on the rows of that stripe whose H is exactly the propagated value hold something smaller in the reference: those
// cells get the taint bit.  fp = F crossing a stripe start, carried down the rows of the stripe; the row loop runs only in the
// steps where some lane holds fp >= 132 or an armed chain (4 - 5 % of k_scan's steps on random DNA, most of them behind a unit's
// overflow cut, where k_scan does not call this any more: scan.hip, q2_past_cut).
//
// All values are carried x SC with the taint in bit SC / 2 (k_scan: SC = 2, bit 0; k_align_fwd<TAINT>: SC = 64, bit 5).  Scores
// and gap costs are multiples of SC, so the bit rides through add / saturating subtract for free.
// F16 (k_scan, SC = 2): H, E and F are f16 integers; the branch converts them and sets a taint by adding 1.0 to a value that is
// still even.  The chain state travels as integers in every build.
//
// recv_f / recv_fp: F and the chain state arriving from virtual lane v - 1.  fpo halves: bits 0..14 = propagated value, bit 15 =
// "an early exit was possible at an earlier row".  live: 0xFFFF in the halves whose column can start or carry a chain (0: void).
// Returns whether the row loop ran.  If so H / E / hbot carry the new taints and fpo the outgoing chain state; else all untouched.
template <int SC, bool F16, int RP>
__device__ __forceinline__ bool q2_rows(int (&H)[RP], int (&E)[RP], int& hbot, int& fpo, int recv_f, int recv_fp, v2u startm, v2u actm,
	uint32_t act, v2u live)
{
	static_assert(!F16 || SC == 2, "the f16 pipe carries 2 x value + taint");
	constexpr int TB = SC == 2 ? 0 : (SC == 64 ? 5 : -1);          // the taint bit SC / 2
	static_assert(TB >= 0, "scale not provided for");
	constexpr uint32_t K1 = 0x00010001u, KGE = (uint32_t)(132 * SC - 1) * 0x10001u, KLT = (uint32_t)(144 * SC) * 0x10001u,
		KE = (uint32_t)(GAP_EXT * SC) * 0x10001u, KO = (uint32_t)(GAP_OPEN * SC) * 0x10001u;
	// cheap superset first (3 VALU): a stripe-start lane receives F >= 132, or some lane receives a live chain;
	// the exact condition is only evaluated behind it
	// (F16: F arrives as f16 bits, and bits(F) > bits(263) iff F > 263)
	const v2u cand = pk_subs_k(u_from(recv_f) & startm, F16 ? f16c2(132 * SC - 1) : KGE) | u_from(recv_fp);
	bool enter = false;
	v2u fp_in = (v2u){ 0, 0 }, arm_in = (v2u){ 0, 0 };
	if (__builtin_amdgcn_ballot_w64(to_int(cand) != 0) != 0ull) {
		const v2u fpraw = ((u_from(F16 ? hf_to_u16(recv_f) : recv_f) & startm) | (u_from(recv_fp) & ~startm)) & live;
		fp_in = fpraw & (v2u){ 0x7fff, 0x7fff };
		arm_in = (fpraw >> (v2u){ 15, 15 }) & ~startm;
		const v2u hot = pk_subs_k(fp_in, KGE) | pk_minu(arm_in, fp_in);
		enter = __builtin_amdgcn_ballot_w64(to_int(hot) != 0) != 0ull;
	}
	if (!enter) return false;
	v2u fp = fp_in, arm = arm_in;
	const v2u one = (v2u){ 1, 1 };
	// pass 1 only READS H and E and collects the taint decisions as bit r of (dh, de)[r / 16]; pass 2 ORs them
	// in.  Every read of the old value thus precedes the in-place update, so H[r] / E[r] stay in the registers
	// the common path uses and the join needs no copies.
	uint32_t dh[2] = { 0u, 0u }, de[2] = { 0u, 0u };
#pragma unroll
	for (int r = 0; r < RP; r++) {
		const v2u hr = u_from(F16 ? hf_to_u16(H[r]) : H[r]), er = u_from(F16 ? hf_to_u16(E[r]) : E[r]);
		const v2u ge = pk_minu_k(pk_subs_k(fp, KGE), K1);                       // Fp >= 132
		// H < 144; a tainted H may be smaller in the reference, so it counts as "< 144" too
		v2u lt = pk_minu_k(pk_ksubs(KLT, hr), K1) | ((hr >> (v2u){ TB, TB }) & one);
		// the reference keeps a smaller H only where, after a possible early exit, H is exactly the propagated value
		v2u eq = pk_ksubs(K1, pk_subs(hr, fp));                                  // H <= Fp (H >= Fp always)
		v2u nfp = pk_subs_k(fp, KE);
		if (r == RP - 1) { lt &= actm; eq &= actm; nfp = (nfp & actm) | (fp & ~actm); }
		const v2u dev = pk_minu(pk_minu(eq, fp), arm);                           // 0 / 1
		// E of this row was just derived from the untainted H: taint it when it came from H (or ties with it)
		const v2u ho = pk_subs_k(hr, KO);
		const v2u efrom = pk_minu(pk_ksubs(K1, pk_subs(er, ho)), ho);
		// (F16: only a value that is still even gets the 1.0; through the asm helper, so that the decision is taken here and
		//  hr / er die with the row: left to the compiler, the and-not is fused into the OR tree below and keeps them alive)
		dh[r >> 4] |= (uint32_t)to_int(F16 ? pk_subs(dev, hr & one) : dev) << (r & 15);
		de[r >> 4] |= (uint32_t)to_int(F16 ? pk_subs(pk_minu(efrom, dev), er & one) : pk_minu(efrom, dev)) << (r & 15);
		arm = pk_maxu(arm, pk_minu(ge, lt));
		fp = nfp;
	}
#pragma unroll
	for (int r = 0; r < RP; r++) {
		if (F16) {
			hf_add_in_place(H[r], (int)(((dh[r >> 4] >> (r & 15)) & K1) * F16_ONE));
			hf_add_in_place(E[r], (int)(((de[r >> 4] >> (r & 15)) & K1) * F16_ONE));
		} else {
			or_in_place(H[r], (int)(((dh[r >> 4] >> (r & 15)) & K1) << TB));
			or_in_place(E[r], (int)(((de[r >> 4] >> (r & 15)) & K1) << TB));
		}
	}
	if (RP > 1) hbot = (H[RP - 1] & (int)act) | (H[RP > 1 ? RP - 2 : 0] & ~(int)act);
	else hbot = H[0];
	fpo = to_int(fp | (arm << (v2u){ 15, 15 }));
	return true;
}

} // namespace fasim
