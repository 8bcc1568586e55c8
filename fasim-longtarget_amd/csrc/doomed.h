// doomed.h -- which candidate alignments of stage 3 are certain to fail the stability filter, decided from their ends alone.  One
// rule for the finish kernels (align.hip) and the host (engine_stage3.cpp, host_post.cpp); no other dependencies.
//
// The record loop (convert_triplex_num, host_post.cpp; fastsim.h:344-383) walks the alignment's columns left to right.  A column is
// M (target letter, strand letter, query letter), D (target letter, strand letter, '-') or I ('-', '-', query letter).  `cur` is
// the display-strand letter of an M or D column and '-' of an I column; prev_c is the `cur` of the last M or D column.  With
// v = triplex_stability(cur, query letter) in [0, 4.5] (0 for every column with a '-'):
//
//     if cur == prev_c == 'T':  tri += -prev_v + penaltyT,  v = penaltyT          (prev_v: the v of the column just before)
//     if cur == prev_c == 'C':  tri += -prev_v + penaltyC,  v = penaltyC
//     tri += v
//
// and tri_score = tri / nt for ntMin <= nt <= ntMax, else 0 (nt = number of columns).
//
// (1) A TT pair inside the span always fires.  The M and D columns of an alignment show the columns ref_begin .. ref_end of the
//     display strand, each once and in order; I columns do not touch prev_c.  So if the strand holds 'T' at columns q and q + 1,
//     both inside [ref_begin, ref_end], the column of q + 1 finds prev_c == 'T' whatever the CIGAR.
// (2) That column adds -prev_v + 2 penaltyT.  The column before it is an I column (prev_v = 0), the T column of q unsubstituted
//     (prev_v >= 0) or substituted (prev_v = penaltyT): with penaltyT < 0 it adds at most penaltyT.
// (3) Every other column adds at most vmax = max(4.5, penaltyC, 0) ON AVERAGE: an unsubstituted one adds v <= 4.5, a T-substituted
//     one at most penaltyT < 0, a C-substituted one -prev_v + 2 penaltyC, which is penaltyC behind a substituted C and at most
//     2 penaltyC together with the column before it (that column added prev_v >= 0 itself and is neither the TT column nor
//     paired with another one).
// Hence tri <= vmax (nt - 1) + penaltyT, and tri_score < minStability is certain when
//
//     vmax (nt - 1) + penaltyT < minStability nt - 1        (the -1: margin for the float accumulation; every term is < 2^24)
//
// for every nt the span allows: max(refspan, readspan) <= nt <= refspan + readspan.  Both sides are linear in nt, so the two ends
// of the range decide.  An nt above ntMax gives tri_score = 0, which fails the filter because minStability > 0.
// With penaltyT >= 0 or minStability <= 0 nothing is certain and the rule answers false.
//
// The drop `total < ntMin` (fastsim.h:385) comes before the de-duplication and must stay exact: length_known() tells when it cannot
// happen.  An alignment is left without its CIGAR only when both functions say yes.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FASIM_HD __host__ __device__
#else
#define FASIM_HD
#endif

namespace fasim {

struct DoomedParams { int penaltyT, penaltyC, ntMin, ntMax; float minStability; };

// The float margin.  With k >= 1 T-substituted columns the real sum is at most vmax (nt - 1) + penaltyT - (k - 1)(|penaltyT| + vmax),
// and |tri| never exceeds vmax nt + 2 k |penaltyT| on the way.  The accumulation makes at most 3 nt roundings of 2^-24 relative
// each, eps = 3 nt 2^-24 in all, so the float sum exceeds the real one by at most eps (vmax nt + 2 k |penaltyT|).  The k - 1 further
// pairs pay for their own share (1 > 2 eps), which leaves eps (vmax nt + 2 |penaltyT|) for the margin of 1 to cover.  With the limits
// below eps < 9.2 * 10^-5 and vmax nt + 2 |penaltyT| <= 8 * 512 + 4000: 0.75.  Outside them the rule answers false.
constexpr long DOOMED_MAX_NT = 512;
constexpr int DOOMED_MAX_PENALTY_T = 2000, DOOMED_MAX_PENALTY_C = 8;

FASIM_HD inline bool doomed_at(const DoomedParams& p, double vmax, long nt)
{
	if (nt > (long)p.ntMax) return true;                                 // tri_score = 0 < minStability
	return vmax * (double)(nt - 1) + (double)p.penaltyT < (double)p.minStability * (double)nt - 1.0;
}

// true only when tri_score < minStability holds for every CIGAR between the given ends
FASIM_HD inline bool stability_doomed(const DoomedParams& p, int refspan, int readspan, bool has_tt)
{
	if (!has_tt || p.penaltyT >= 0 || !(p.minStability > 0.0f) || refspan < 1 || readspan < 1) return false;
	if (p.penaltyT < -DOOMED_MAX_PENALTY_T || p.penaltyC > DOOMED_MAX_PENALTY_C) return false;
	double vmax = 4.5;
	if ((double)p.penaltyC > vmax) vmax = (double)p.penaltyC;
	const long lo = refspan > readspan ? refspan : readspan, hi = (long)refspan + (long)readspan;
	if (hi > DOOMED_MAX_NT) return false;
	return doomed_at(p, vmax, lo) && doomed_at(p, vmax, hi);
}

// true when the alignment's column count cannot be below ntMin
FASIM_HD inline bool length_known(int ntMin, int refspan, int readspan) { return (refspan > readspan ? refspan : readspan) >= ntMin; }

// strand shown in the TTS column by encoding enc in [0, 48): 1 = complement of the segment (enc_info, host_post.cpp)
FASIM_HD inline int enc_strand(int enc) { return enc < 12 ? (enc & 1) : (((enc - 12) & 1) ? 0 : 1); }

// Does the display strand of a unit hold 'T' at two adjacent unit columns inside [q0, q1]?  seg: the segment's n letters; unit column
// q shows seg[q], or seg[n - 1 - q] under an odd (reversed) encoding, complemented when the encoding's strand is 1 (a 'T' is then an
// 'A' of the segment).  Only for segments without letters that complement() drops, or strand 0.  q0 >= 0 and q1 < n.
FASIM_HD inline bool span_has_tt(const unsigned char* seg, int n, int enc, int q0, int q1)
{
	const unsigned char t = enc_strand(enc) == 1 ? 'A' : 'T';
	const bool rev = (enc & 1) != 0;
	bool prev = false;
	for (int q = q0; q <= q1; q++) {
		const bool is = seg[rev ? n - 1 - q : q] == t;
		if (is && prev) return true;
		prev = is;
	}
	return false;
}

} // namespace fasim
