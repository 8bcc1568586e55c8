// tests/doomed_main.cpp -- stand-alone driver of csrc/doomed.h for tests/test_doomed_cpu.py: random alignments (ends + CIGAR) over random
// segments go through the scan's own record conversion (convert_triplex_num, host_post.cpp) and through the rule; the driver counts
// where the two disagree.  Plain host C++, no HIP.  Build: c++ doomed_main.cpp ../fasim-longtarget_amd/csrc/host_post.cpp -lpthread
//
//   doomed_main SEED TRIALS    one line per parameter set:
//     set PT PC MINS NTMIN NTMAX cases N rule R stab_miss A len_known K len_miss B coord_miss C kind_miss D
//   PT/PC/MINS/NTMIN/NTMAX: penaltyT, penaltyC, minStability, ntMin, ntMax;  R: alignments the rule calls doomed;  A: of those, records
//   with tri_score >= minStability;  K: length_known answers yes;  B: of those, alignments that left no record (total < ntMin);
//   C: doomed alignments whose push_doomed_num record differs from the converted one in a field the de-duplication reads;
//   D: planted cases whose TT test came out wrong (kinds 1, 2, 5 must say no; 3, 4 yes).
// and first a line "strand_miss S": encodings whose enc_strand differs from enc_info.
#include "../fasim-longtarget_amd/csrc/doomed.h"
#include "../fasim-longtarget_amd/csrc/host_post.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace fasim;

struct Case { std::string seg; int enc; AlignResult al; std::vector<uint32_t> cigar; int kind; };

static std::mt19937_64 rng;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

// segment index of unit column q, and the segment letter that shows as `disp` there
static int seg_index(int n, int enc, int q) { return (enc & 1) ? n - 1 - q : q; }
static char seg_letter(int enc, char disp)
{
	if (enc_info(enc).strand != 1) return disp;
	switch (disp) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; default: return 'A'; }
}
static void show(Case& c, int q, char disp) { if (q >= 0 && q < (int)c.seg.size()) c.seg[seg_index((int)c.seg.size(), c.enc, q)] = seg_letter(c.enc, disp); }

// kinds: 0 random; 1 the only TT straddles ref_begin - 1 / ref_begin; 2 ... ref_end / ref_end + 1; 3 TT inside with an I run between
// the two columns; 4 TT inside, the second T under a D column; 5 no T in the span
static Case make_case()
{
	Case c;
	c.kind = rnd(0, 9) < 5 ? 0 : rnd(1, 5);
	c.enc = rnd(0, 47);
	const int n = rnd(130, 400);
	const char* alphabet = rnd(0, 3) ? "ACGT" : "ATTT";      // T-rich segments too: both strands show TT often
	c.seg.resize(n);
	for (int i = 0; i < n; i++) c.seg[i] = alphabet[rnd(0, 3)];
	const bool dirty = c.kind == 0 && rnd(0, 4) == 0;
	if (dirty) for (int k = rnd(1, 6); k > 0; k--) c.seg[rnd(0, n - 1)] = "NRYn"[rnd(0, 3)];
	const int refspan = c.kind >= 3 && c.kind <= 4 ? rnd(3, 120) : rnd(1, 120);
	const int rb = rnd(c.kind == 1 ? 1 : 0, n - refspan - (c.kind == 2 ? 1 : 0));
	const int re = rb + refspan - 1;
	int tq = -1;                                                // kinds 3, 4: display columns tq, tq + 1 hold the pair
	if (c.kind != 0) {
		const char* others = "ACG";
		for (int q = rb - 1; q <= re + 1; q++) show(c, q, others[rnd(0, 2)]);
		if (c.kind == 1) { show(c, rb - 1, 'T'); show(c, rb, 'T'); }
		if (c.kind == 2) { show(c, re, 'T'); show(c, re + 1, 'T'); }
		if (c.kind == 3 || c.kind == 4) { tq = rnd(rb, re - 2); show(c, tq, 'T'); show(c, tq + 1, 'T'); }
	}
	// CIGAR over the reference span: runs of M / D that consume it, I runs in between; first and last column M
	std::vector<int> ops;                                      // one op per column
	for (int q = rb; q <= re; q++) {
		int op = 0;
		if (q > rb && q < re && rnd(0, 9) == 0) op = 2;
		if (c.kind == 4 && q == tq + 1) op = 2;
		if (c.kind == 4 && q == tq) op = 0;
		ops.push_back(op);
		const bool force_i = c.kind == 3 && q == tq;
		if (q < re && (force_i || rnd(0, 14) == 0)) for (int k = rnd(1, 4); k > 0; k--) ops.push_back(1);
	}
	int readspan = 0;
	for (int op : ops) if (op != 2) readspan++;
	if (readspan > 120) {                                       // keep the query span within 1-120: drop I columns from the end
		for (size_t k = ops.size(); k-- > 0 && readspan > 120; ) if (ops[k] == 1 && !(c.kind == 3)) { ops.erase(ops.begin() + (long)k); readspan--; }
	}
	for (size_t k = 0; k < ops.size(); ) {
		size_t e = k;
		while (e < ops.size() && ops[e] == ops[k]) e++;
		c.cigar.push_back((uint32_t)((e - k) << 4) | (uint32_t)ops[k]);
		k = e;
	}
	c.al.ref_begin = rb; c.al.ref_end = re;
	c.al.query_begin = rnd(0, 200); c.al.query_end = c.al.query_begin + readspan - 1;
	c.al.sw_score = rnd(30, 147); c.al.cigar_len = (int)c.cigar.size();
	return c;
}

int main(int argc, char** argv)
{
	if (argc < 3) { fprintf(stderr, "usage: doomed_main SEED TRIALS\n"); return 2; }
	const uint64_t seed = strtoull(argv[1], nullptr, 10);
	const int trials = atoi(argv[2]);
	int strand_miss = 0;
	for (int enc = 0; enc < 48; enc++) if (enc_strand(enc) != enc_info(enc).strand) strand_miss++;
	printf("strand_miss %d\n", strand_miss);
	rng.seed(seed);
	std::string rna(400, 'A');
	for (char& ch : rna) ch = "ACGT"[rnd(0, 3)];
	std::vector<Case> cases;
	for (int t = 0; t < trials; t++) cases.push_back(make_case());

	struct Set { int pT, pC; float minS; int ntMin, ntMax; };
	std::vector<Set> sets;
	const int pTs[4] = { -1000, -1, 0, 5 }, pCs[3] = { 0, -3, 6 };
	const float minSs[3] = { 0.0f, 1.0f, 4.6f };
	for (int a : pTs) for (float b : minSs) for (int c : pCs) sets.push_back({ a, c, b, 20, 100000 });
	sets.push_back({ -1000, 0, 1.0f, 20, 30 });                  // ntMax small: longer alignments have tri_score 0
	sets.push_back({ -1000, 0, 1.0f, 1, 100000 });               // ntMin 1: every alignment is a record
	sets.push_back({ -1000, 0, 1.0f, 60, 100 });
	sets.push_back({ -5000, 0, 1.0f, 20, 100000 });              // a penalty beyond the limit of the float argument
	for (const Set& s : sets) {
		fasim_params p;
		memset(&p, 0, sizeof p);                                   // (the conversion reads the five fields below only)
		p.penaltyT = s.pT; p.penaltyC = s.pC; p.minStability = s.minS; p.ntMin = s.ntMin; p.ntMax = s.ntMax;
		const DoomedParams dp{ s.pT, s.pC, s.ntMin, s.ntMax, s.minS };
		long rule = 0, stab_miss = 0, len_known = 0, len_miss = 0, coord_miss = 0, kind_miss = 0;
		for (const Case& c : cases) {
			const int n = (int)c.seg.size();
			const bool acgtn = only_acgtn(c.seg.data(), n);
			const int refspan = c.al.ref_end - c.al.ref_begin + 1, readspan = c.al.query_end - c.al.query_begin + 1;
			// the kernel's rule: never where complement() drops letters (strand 1 of a segment with letters outside ACGTN)
			const bool usable = acgtn || enc_strand(c.enc) != 1;
			const bool has_tt = usable && span_has_tt((const unsigned char*)c.seg.data(), n, c.enc, c.al.ref_begin, c.al.ref_end);
			if (c.kind != 0 && has_tt != (c.kind == 3 || c.kind == 4)) kind_miss++;
			std::vector<TriplexNum> rec;
			convert_triplex_num(c.al, c.cigar.data(), rna, c.seg.data(), n, c.enc, 7000, p, rec, acgtn);
			if (length_known(s.ntMin, refspan, readspan)) { len_known++; if (rec.empty()) len_miss++; }
			if (!stability_doomed(dp, refspan, readspan, has_tt)) continue;
			rule++;
			if (rec.empty()) continue;
			if (!(rec[0].tri_score < s.minS)) stab_miss++;
			std::vector<TriplexNum> mine;
			push_doomed_num(c.al, n, c.enc, 7000, mine);
			const TriplexNum& a = rec[0]; const TriplexNum& b = mine[0];
			if (a.stari != b.stari || a.endi != b.endi || a.starj != b.starj || a.endj != b.endj || a.score != b.score || (b.nt < s.ntMin && length_known(s.ntMin, refspan, readspan))) coord_miss++;
		}
		printf("set %d %d %g %d %d cases %zu rule %ld stab_miss %ld len_known %ld len_miss %ld coord_miss %ld kind_miss %ld\n", s.pT, s.pC, (double)s.minS,
			s.ntMin, s.ntMax, cases.size(), rule, stab_miss, len_known, len_miss, coord_miss, kind_miss);
	}
	return 0;
}
