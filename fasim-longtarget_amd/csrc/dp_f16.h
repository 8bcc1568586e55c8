// Packed-f16 form of the Gotoh row pair (scan.hip, align.hip) for gfx950.
//
// Every value the two systolic kernels carry is a small non-negative integer, and f16 holds every integer of magnitude
// <= 2048 exactly, so inside that range f16 adds and maxima compute the very integers the packed 16-bit integer ops
// compute.  What f16 buys is v_pk_maximum3_f16 (there is no packed integer max3): the row pair
//     t = Hdiag + sc ; h = max3(t, E, F) ; ho = h - open ; E = max3(E - ext, ho, 0) ; F = max3(F - ext, ho, 0)
// is 8 instructions (plus the perm, and half a max3 for the lane maximum) instead of 10, at the same issue cost per
// instruction (profiles/r07_valu_issue_bench_f16.txt).  The third operand 0 is the floor the saturating integer
// subtraction gave for free.  Non-negative f16 order like their bit patterns read as u16, so masks, the column-maximum
// chain and the superset test of the hazard branch stay integer ops on the same registers.
//
// Exactness: sums and differences of integers are exact while the result stays within +-2048; nothing lies in (0, 1), so
// neither the rounding nor the denormal mode matters; x - x is +0 under round-to-nearest and the floor operand is +0, so
// no -0 arises (maximum3 orders -0 < +0).  No NaN arises: the only infinity is the deliberate "minus +inf" that clears
// E and F in void columns (align.hip), and it only ever meets finite values.
//
// All helpers are inline asm: the instruction count is the whole point, and the tied operands keep the H column in place
// from step to step (see scan.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fasim {

// f16 bits of a small integer (exact for |x| <= 2048), and back (values the pipe hands out are non-negative integers)
__device__ __forceinline__ uint16_t f16_bits(int x) { return __builtin_bit_cast(uint16_t, (_Float16)(float)x); }
__device__ __forceinline__ uint32_t f16_bits2(int x) { return (uint32_t)f16_bits(x) * 0x10001u; }
__device__ __forceinline__ uint32_t f16_int(uint32_t half_bits) { return (uint32_t)(float)__builtin_bit_cast(_Float16, (uint16_t)half_bits); }
// a packed pair of f16 integers -> the packed pair of u16 integers
__device__ __forceinline__ uint32_t f16_pair_int(uint32_t x) { return f16_int(x & 0xffffu) | (f16_int(x >> 16) << 16); }
// compile-time f16 bits of a non-negative integer < 2048
constexpr uint32_t f16c(uint32_t v)
{
	if (v == 0) return 0u;
	int e = 0;
	while ((v >> (e + 1)) != 0) e++;
	return ((uint32_t)(e + 15) << 10) | ((v << (10 - e)) & 0x3FFu);
}
constexpr uint32_t f16c2(uint32_t v) { return f16c(v) * 0x10001u; }
constexpr uint32_t F16_ONE = 0x3C00u, F16_INF2 = 0x7C007C00u, F16_2048 = 0x6800u;

// sc += hold, in the register of the score (which dies there)
__device__ __forceinline__ int hf_diag_plus_score(int hold, int sc) { asm("v_pk_add_f16 %0, %1, %0" : "+v"(sc) : "v"(hold)); return sc; }
// new H = max3(t, e, f), written into the register of the OLD H (tied dummy operand); `after` is an unused operand that only
// orders this behind the sum for the next row, which still reads the old H
__device__ __forceinline__ int hf_h(int hold, int t, int e, int f, int after)
{
	int hn;
	asm("v_pk_maximum3_f16 %0, %2, %3, %4" : "=v"(hn) : "0"(hold), "v"(t), "v"(e), "v"(f), "v"(after));
	return hn;
}
// a - k (k: packed f16 constant in a scalar register, or a per-lane register)
__device__ __forceinline__ int hf_sub_k(int a, uint32_t k) { int r; asm("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "s"(k)); return r; }
__device__ __forceinline__ int hf_sub(int a, int b) { int r; asm("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
// max3(a, b, +0)
__device__ __forceinline__ int hf_max_floor(int a, int b) { int r; asm("v_pk_maximum3_f16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ int hf_max3(int a, int b, int c) { int r; asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// x += y in place (rare branches: a value they may change then needs no copy at the join with the common path)
__device__ __forceinline__ void hf_add_in_place(int& x, int y) { asm volatile("v_pk_add_f16 %0, %0, %1" : "+v"(x) : "v"(y)); }

} // namespace fasim
