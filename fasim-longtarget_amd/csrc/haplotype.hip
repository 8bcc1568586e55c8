// fasim-longtarget_amd/csrc/haplotype.hip -- k_hap_encode: the target codes of allele windows written in the letters of the record or
// of a haplotype, for gfx950 (DESIGN.md sections 19 and 25).
//
// The window of a variant on a haplotype is the record with the haplotype's other variants applied, which nobody materialises: the
// host describes it as pieces (stretches of the record and of uploaded ALT strings) with their running ends.  The plain window of
// section 19 -- flank, allele, flank -- is the same thing in at most three pieces, so this kernel encodes those as well.  One workgroup
// per problem (window x encoding): the first HAP_LDS_PIECES ends of the window are staged in LDS, every thread maps its
// column (mirrored for an odd encoding) to a piece and an offset by binary search -- in LDS, or in HBM for the pieces behind the
// stage -- fetches the letter and writes its code: tcodes[tbase + c] is the code of window letter c, or of letter n - 1 - c
// for an odd encoding, which is what k_touch and k_touch_reduce (variant.hip) read.  Plain vector stores only, one writer per byte, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace fasim {

constexpr int HE_THREADS = 256;

__global__ void __launch_bounds__(HE_THREADS) k_hap_encode(HapEncodeLaunch a)
{
	__shared__ int32_t ends_sh[HAP_LDS_PIECES];
	const int p = blockIdx.x;
	if (p >= a.nprob) return;
	const TouchProb P = a.probs[p];
	const HapWindow W = a.wins[P.win];
	const int32_t* ends = a.ends + W.piece0;
	const HapPiece* pieces = a.pieces + W.piece0;
	const int staged = min(W.npiece, HAP_LDS_PIECES);
	for (int k = threadIdx.x; k < staged; k += HE_THREADS) ends_sh[k] = ends[k];
	__syncthreads();
	if (W.npiece < 1 || P.n < 1 || P.n > TOUCH_MAX_COLS) return;      // (uniform)
	const uint8_t* lut = a.enc_lut + P.enc * 256;
	const int staged_end = ends_sh[staged - 1];      // window letters that the staged pieces cover
	for (int c = threadIdx.x; c < P.n; c += HE_THREADS) {
		const int j = (P.enc & 1) ? P.n - 1 - c : c;
		// the piece of letter j: the first one whose end lies above j
		int lo, hi;
		if (j < staged_end) {
			lo = 0; hi = staged - 1;
			while (lo < hi) { const int mid = (lo + hi) >> 1; if (ends_sh[mid] > j) hi = mid; else lo = mid + 1; }
		} else {
			lo = staged; hi = W.npiece - 1;
			while (lo < hi) { const int mid = (lo + hi) >> 1; if (ends[mid] > j) hi = mid; else lo = mid + 1; }
			lo = min(lo, W.npiece - 1);
		}
		const int first = lo == 0 ? 0 : (lo <= staged ? ends_sh[lo - 1] : ends[lo - 1]);
		const HapPiece Q = pieces[lo];
		const uint8_t letter = (Q.alt ? a.alts : a.dna)[Q.src + (j - first)];
		a.tcodes[P.tbase + c] = lut[letter];
	}
}

hipError_t launch_hap_encode(const HapEncodeLaunch& L, hipStream_t st)
{
	if (L.nprob <= 0) return hipSuccess;
	if (!L.dna || !L.alts || !L.wins || !L.pieces || !L.ends || !L.probs || !L.enc_lut || !L.tcodes) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_hap_encode, dim3((unsigned)L.nprob), dim3(HE_THREADS), 0, st, L);
	return hipGetLastError();
}

} // namespace fasim
