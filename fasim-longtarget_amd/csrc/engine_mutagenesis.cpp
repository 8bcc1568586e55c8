// fasim-longtarget_amd/csrc/engine_mutagenesis.cpp -- fasim_score_mutagenesis: every substitution at every position of an interval,
// scored by the triplex potential through it from one shared pass (kernels: haplotype.hip, mutagenesis.hip), and
// the table of `fasim --mutagenesis` (fasim_mutagenesis_tsv); fasim_score_deletions and fasim_deletions_tsv, the same for every
// deletion inside an interval (section 27, at the end of the file).
//
// The work of a query is cut into launches of groups.  A group is one range of an interval's positions under all enabled encodings:
// its context goes to k_hap_encode as a window of one piece, every encoding of it is a unit of k_mut_prefix, and every (position,
// letter, encoding) a problem of k_mut_touch.  A launch takes groups, and of the last one as many positions as fit, until a fixed
// bound on the snapshots' bytes, on the HBM row state of long queries, on the problems or on the target codes is reached; a range that
// does not start its interval runs its prefix from column 0 again.  Every position belongs to one group and a group's result does not
// look at another's, so the cuts cannot show.  A launch is: the groups up, k_hap_encode, k_mut_prefix, k_mut_touch, k_mut_reduce,
// twenty words per position back.  Everything runs on the engine's own stream, in the chunk buffers of section 19 (vr_*) and four of
// its own (mu_*): the engine's query, its scan buffers and its workers are not touched.
#include "engine.h"

namespace {

constexpr size_t MU_SNAP_BYTES = (size_t)256 << 20;      // snapshots of a launch
constexpr size_t MU_ROW_BYTES = (size_t)256 << 20;       // HBM row state of a launch (queries above TOUCH_LDS_ROWS)
constexpr int64_t MU_MAX_PROBS = 1 << 20;                // problems of a launch
constexpr size_t MU_TCODE_BYTES = (size_t)16 << 20;      // target codes of a launch

inline int pad16(int n) { return (n + 15) & ~15; }

inline int ref_index(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

struct Context { int64_t lo, hi; };
inline Context context_of(const fasim_interval& I, int64_t len, int32_t flank) { return { std::max<int64_t>(0, I.start - flank), std::min<int64_t>(len, I.end + flank) }; }

// HIP-event seconds of the two kernels of a launch
struct KernelClock {
	fasim_engine* E; hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
	explicit KernelClock(fasim_engine* e) : E(e) { for (hipEvent_t& x : ev) x = get_event(E); }
	~KernelClock() { for (hipEvent_t x : ev) if (x) E->ev_pool.push_back(x); }
	void mark(int k) { if (ev[k]) (void)hipEventRecord(ev[k], E->st); }
	double seconds(int a, int b) const { float ms = 0.0f; return ev[a] && ev[b] && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess ? ms * 1e-3 : 0.0; }
};

}  // namespace

int fasim_score_mutagenesis(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_interval* ivs, int64_t nint, int32_t flank,
	const fasim_params* pp, fasim_mut_score* out, fasim_mutagenesis_stats* stats)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nint < 0 || (nint > 0 && (!ivs || !out))) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_variant_call(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, flank, pp, rs); if (rc) return rc;
	int64_t npos = 0;
	for (int64_t k = 0; k < nint; k++) {
		const fasim_interval& I = ivs[k];
		if (I.rec < 0 || I.rec >= nrec) return fail(E, FASIM_E_ARG, "interval %lld: record %d of %d", (long long)k, I.rec, nrec);
		if (I.start < 0 || I.end <= I.start || I.end > rec_len[I.rec])
			return fail(E, FASIM_E_ARG, "interval %lld: [%lld, %lld) is no stretch of record %d of %lld nt", (long long)k, (long long)I.start, (long long)I.end, I.rec, (long long)rec_len[I.rec]);
		if (I.end - I.start + 2 * (int64_t)flank > TOUCH_MAX_COLS)
			return fail(E, FASIM_E_ARG, "interval %lld: %lld positions and two flanks of %d are more than %d columns", (long long)k, (long long)(I.end - I.start), flank, TOUCH_MAX_COLS);
		npos += I.end - I.start;
	}
	const double t0 = now_s();
	fasim_mutagenesis_stats st;
	memset(&st, 0, sizeof st);
	st.intervals = nint; st.positions = npos;
	const char* host = rs.host(E);
	for (int q = 0; q < nq; q++) {
		fasim_mut_score* row = out + (size_t)q * (size_t)npos;
		int64_t at = 0;
		for (int64_t k = 0; k < nint; k++) for (int64_t x = ivs[k].start; x < ivs[k].end; x++) {
			fasim_mut_score& s = row[at++];
			memset(&s, 0, sizeof s);
			memset(s.enc, -1, sizeof s.enc);
			s.ref = (int8_t)ref_index(host[rec_off[ivs[k].rec] + x]);
		}
	}
	const std::vector<int> encs = enabled_encodings(*pp);
	const int nenc = (int)encs.size();
	if (npos == 0 || nenc == 0) { st.total_s = now_s() - t0; if (stats) *stats = st; return FASIM_OK; }
	HIPOK(hipSetDevice(E->device));
	try {
		for (int q = 0; q < nq; q++) {
			const int m = rna_lens[q];
			std::vector<uint8_t> qc((size_t)m);
			for (int i = 0; i < m; i++) qc[(size_t)i] = code2(rnas[q][i]);
			rc = upload(E, E->vr_q, qc.data(), qc.size()); if (rc) return rc;
			const bool rows_hbm = m > TOUCH_LDS_ROWS;
			const size_t state_rows = (size_t)touch_state_rows(m), row_bytes = 6 * state_rows, snap_bytes = 4 * state_rows;
			// what one more position costs a launch, in positions: the tightest of the three bounds
			const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(MU_MAX_PROBS / (4 * nenc), std::min<int64_t>((int64_t)(MU_SNAP_BYTES / (snap_bytes * (size_t)nenc)),
				rows_hbm ? (int64_t)(MU_ROW_BYTES / (row_bytes * 4 * (size_t)nenc)) : INT64_MAX)));
			fasim_mut_score* row = out + (size_t)q * (size_t)npos;
			int64_t it = 0, x = 0, gpos = 0;      // the next position: offset x of interval it, the call's position gpos
			while (it < nint) {
				std::vector<HapWindow> wins; std::vector<HapPiece> pieces; std::vector<int32_t> ends, first;
				std::vector<TouchProb> units; std::vector<MutGroup> groups; std::vector<uint8_t> letters;
				size_t tbytes = 0;
				int64_t lpos = 0;
				const int64_t gpos0 = gpos;
				while (it < nint) {
					const fasim_interval& I = ivs[it];
					const Context C = context_of(I, rec_len[I.rec], flank);
					const int n = (int)(C.hi - C.lo);
					const size_t need = (size_t)nenc * (size_t)pad16(n);
					if (lpos > 0 && (lpos >= cap || tbytes + need > MU_TCODE_BYTES)) break;
					const int64_t take = std::min<int64_t>(I.end - I.start - x, cap - lpos);
					HapPiece D; D.pad = 0; D.alt = 0; D.src = rec_off[I.rec] + C.lo;
					if (!rs.resident) { D.src = (int64_t)letters.size(); letters.insert(letters.end(), dna + rec_off[I.rec] + C.lo, dna + rec_off[I.rec] + C.hi); }
					HapWindow H; H.piece0 = (int64_t)pieces.size(); H.npiece = 1; H.pad = 0;
					pieces.push_back(D); ends.push_back(n);
					MutGroup G; G.unit0 = (int32_t)units.size(); G.pos0 = (int32_t)lpos; G.npos = (int32_t)take; G.pad = 0;
					const int a0 = (int)(I.start - C.lo + x), a1 = a0 + (int)take;
					const int edge_lo = C.lo > 0, edge_hi = C.hi < rec_len[I.rec];
					for (int k = 0; k < nenc; k++) {
						TouchProb P; P.tbase = (int64_t)tbytes; P.n = n; P.win = (int32_t)wins.size(); P.enc = encs[(size_t)k];
						if (P.enc & 1) { P.v0 = n - a1; P.v1 = n - a0; P.edge = edge_hi | (edge_lo << 1); }
						else { P.v0 = a0; P.v1 = a1; P.edge = edge_lo | (edge_hi << 1); }
						first.push_back((int32_t)(lpos * nenc + (int64_t)k * take));
						units.push_back(P);
						tbytes += (size_t)pad16(n);
						st.prefix_cols += P.v1 - 1;
						st.cont_cols_bound += 4 * take * n - 2 * take * (P.v0 + P.v1 - 1);
					}
					wins.push_back(H); groups.push_back(G);
					lpos += take; x += take;
					if (x == I.end - I.start) { it++; x = 0; }
				}
				gpos += lpos;
				const int nunit = (int)units.size(), ncol = (int)(lpos * nenc), nprob = 4 * ncol;
				first.push_back(ncol);
				st.launches++; st.prefix_problems += nunit; st.problems += nprob;
				if (E->vr_hwins.ensure(wins.size() * sizeof(HapWindow)) != hipSuccess || E->vr_pieces.ensure(pieces.size() * sizeof(HapPiece)) != hipSuccess ||
					E->vr_ends.ensure(ends.size() * sizeof(int32_t)) != hipSuccess || E->vr_probs.ensure((size_t)nunit * sizeof(TouchProb)) != hipSuccess ||
					E->mu_first.ensure(first.size() * sizeof(int32_t)) != hipSuccess || E->mu_groups.ensure(groups.size() * sizeof(MutGroup)) != hipSuccess ||
					E->vr_alt.ensure(1) != hipSuccess || E->vr_tcodes.ensure(tbytes) != hipSuccess || E->mu_snap.ensure((size_t)ncol * snap_bytes) != hipSuccess ||
					E->vr_touch.ensure((size_t)nprob * sizeof(uint32_t)) != hipSuccess || E->mu_cols.ensure((size_t)nprob * sizeof(uint32_t)) != hipSuccess ||
					E->vr_out.ensure((size_t)lpos * MUT_WORDS * sizeof(uint32_t)) != hipSuccess || (!rs.resident && E->vr_dna.ensure(letters.size() + 1) != hipSuccess) ||
					(rows_hbm && E->vr_rows.ensure((size_t)nprob * row_bytes) != hipSuccess)) {
					(void)hipGetLastError();
					return fail(E, FASIM_E_NOMEM, "mutagenesis: no device memory for a launch of %d problems", nprob);
				}
				HIPOK(hipMemcpyAsync(E->vr_hwins.p, wins.data(), wins.size() * sizeof(HapWindow), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_pieces.p, pieces.data(), pieces.size() * sizeof(HapPiece), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_ends.p, ends.data(), ends.size() * sizeof(int32_t), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_probs.p, units.data(), (size_t)nunit * sizeof(TouchProb), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->mu_first.p, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->mu_groups.p, groups.data(), groups.size() * sizeof(MutGroup), hipMemcpyHostToDevice, E->st));
				if (!rs.resident) HIPOK(hipMemcpyAsync(E->vr_dna.p, letters.data(), letters.size(), hipMemcpyHostToDevice, E->st));
				HapEncodeLaunch EL;
				EL.dna = rs.resident ? E->dna_res.as<uint8_t>() : E->vr_dna.as<uint8_t>(); EL.alts = E->vr_alt.as<uint8_t>(); EL.wins = E->vr_hwins.as<HapWindow>();
				EL.pieces = E->vr_pieces.as<HapPiece>(); EL.ends = E->vr_ends.as<int32_t>();
				EL.probs = E->vr_probs.as<TouchProb>(); EL.nprob = nunit; EL.enc_lut = E->enc_lut.as<uint8_t>(); EL.tcodes = E->vr_tcodes.as<uint8_t>();
				hipError_t he = launch_hap_encode(EL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "mutagenesis (encode) launch failed: %s", hipGetErrorString(he));
				MutLaunch ML;
				ML.tcodes = E->vr_tcodes.as<uint8_t>(); ML.qcodes = E->vr_q.as<uint8_t>(); ML.m = m; ML.units = E->vr_probs.as<TouchProb>();
				ML.first = E->mu_first.as<int32_t>(); ML.nunit = nunit; ML.ncol = ncol; ML.enc_lut = E->enc_lut.as<uint8_t>();
				ML.rows = rows_hbm ? E->vr_rows.as<uint16_t>() : nullptr; ML.snap = E->mu_snap.as<uint16_t>();
				ML.out = E->vr_touch.as<uint32_t>(); ML.cols = E->mu_cols.as<uint32_t>();
				KernelClock clock(E);
				clock.mark(0); he = launch_mut_prefix(ML, E->st); clock.mark(1);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "mutagenesis (prefix) launch failed: %s", hipGetErrorString(he));
				clock.mark(2); he = launch_mut_touch(ML, E->st); clock.mark(3);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "mutagenesis (touch) launch failed: %s", hipGetErrorString(he));
				MutReduceLaunch RL;
				RL.touch = E->vr_touch.as<uint32_t>(); RL.cols = E->mu_cols.as<uint32_t>(); RL.first = E->mu_first.as<int32_t>(); RL.groups = E->mu_groups.as<MutGroup>();
				RL.ngroup = (int32_t)groups.size(); RL.npos = (int32_t)lpos; RL.nenc = nenc; RL.out = E->vr_out.as<uint32_t>();
				memset(RL.enc, 0, sizeof RL.enc);
				for (int k = 0; k < nenc; k++) RL.enc[k] = (uint8_t)encs[(size_t)k];
				he = launch_mut_reduce(RL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "mutagenesis (reduce) launch failed: %s", hipGetErrorString(he));
				std::vector<uint32_t> words((size_t)lpos * MUT_WORDS);
				HIPOK(hipMemcpyAsync(words.data(), E->vr_out.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
				HIPOK(hipStreamSynchronize(E->st));
				st.prefix_s += clock.seconds(0, 1); st.cont_s += clock.seconds(2, 3);
				for (int64_t k = 0; k < lpos; k++) {
					fasim_mut_score& s = row[gpos0 + k];
					const uint32_t* w = &words[(size_t)k * MUT_WORDS];
					for (int b = 0; b < 4; b++) {
						uint32_t top = 0;
						for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
							const uint32_t v = w[b * 4 + c];
							s.value[b][c] = (int32_t)(v >> 9);
							s.enc[b][c] = (v >> 9) ? (int8_t)(v & 0xff) : (int8_t)-1;
							top = std::max(top, v >> 8);
						}
						s.clipped[b] = (uint8_t)(top & 1);
						st.cont_cols += w[16 + b];
					}
				}
			}
		}
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	st.total_s = now_s() - t0;
	if (stats) *stats = st;
	return FASIM_OK;
}

int fasim_mutagenesis_tsv(const fasim_region* regions, const int64_t* offsets, int64_t n, const fasim_mut_score* scores, int32_t flank,
	const char* rna_name, char** text, int64_t* text_len)
{
	if (n < 0 || !rna_name || !text || !text_len || (n > 0 && (!regions || !offsets))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "# fasim mutagenesis lncRNA="; o += rna_name; o += " flank="; o += std::to_string(flank); o += "\n";
	o += "line\tchrom\tpos\tid\tref\talt";
	for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "_ref\t"; o += c; o += "_alt"; }
	o += "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n";
	for (int64_t k = 0; k < n; k++) {
		const fasim_region& g = regions[k];
		if (!g.chrom || !g.name) return fail(nullptr, FASIM_E_ARG, "interval %lld lacks a string", (long long)k);
		const int64_t np = offsets[k + 1] - offsets[k];
		if (np == 0) continue;
		if (np != g.end - g.start || !scores) return fail(nullptr, FASIM_E_ARG, "interval %lld: %lld scores for %lld positions", (long long)k, (long long)np, (long long)(g.end - g.start));
		for (int64_t j = 0; j < np; j++) {
			const fasim_mut_score& s = scores[offsets[k] + j];
			if (s.ref < 0 || s.ref > 3) continue;
			int top[4], rule[4];
			for (int b = 0; b < 4; b++) {
				top[b] = 0; rule[b] = -1;
				for (int c = 0; c < FASIM_TRACK_CLASSES; c++) if (s.value[b][c] > top[b]) { top[b] = s.value[b][c]; rule[b] = (s.enc[b][c] >= 0 && s.enc[b][c] < 48) ? enc_info(s.enc[b][c]).rule : -1; }
			}
			const int r = s.ref;
			for (int b = 0; b < 4; b++) {
				if (b == r) continue;
				o += std::to_string(g.line); o += "\t"; o += g.chrom; o += "\t"; o += std::to_string(g.start + j + 1); o += "\t"; o += g.name;
				o += "\t"; o += "ACGT"[r]; o += "\t"; o += "ACGT"[b];
				for (int c = 0; c < FASIM_TRACK_CLASSES; c++) { o += "\t"; o += std::to_string(s.value[r][c]); o += "\t"; o += std::to_string(s.value[b][c]); }
				o += "\t"; o += std::to_string(top[r]); o += "\t"; o += std::to_string(top[b]); o += "\t"; o += std::to_string(top[b] - top[r]);
				for (int a : { r, b }) { o += "\t"; o += (top[a] > 0 && rule[a] >= 0) ? std::to_string(rule[a]) : std::string("NA"); }
				// the bit of the larger of the two letters' words; the maximum is taken on the doubled integer, so ties go to the bit
				o += "\t"; o += std::to_string(std::max(2 * top[r] + (s.clipped[r] & 1), 2 * top[b] + (s.clipped[b] & 1)) & 1); o += "\n";
			}
		}
	}
	return text_out(o, text, text_len);
}

// ---- every deletion of an interval (kernels: k_mut_prefix_pm, k_mut_jump, k_mut_del_reduce) -----------------------
// The same launches of groups, with three differences.  A group's units cover `next` positions: the range's own and, for the deletions
// that end beyond it, up to the longest length more, never past the interval's end -- so a range cut inside an interval computes the
// snapshots, column maxima and own-letter problems of its neighbour's first positions again and no group looks at another's results.
// A position costs (1 + nlen) * nenc problem slots and the extension nenc snapshot columns each, which the same fixed bounds count;
// a call in which one position alone -- its (1 + longest length) snapshot columns per encoding, never more than its interval has --
// would not fit a launch is refused before any GPU work, so no launch is larger than the bounds.  And ten words per (position, length)
// come back.
namespace {

// positions of the group that starts `done` positions into an interval of `len`: its own `take` and the extension
inline int64_t del_next(int64_t take, int64_t done, int64_t len, int dmax) { return std::min<int64_t>(take + dmax, len - done); }

inline bool clean_run(const char* s, int64_t n) { for (int64_t i = 0; i < n; i++) if (ref_index(s[i]) < 0) return false; return true; }

int check_lengths(fasim_engine* E, const int32_t* lengths, int32_t nlen)
{
	if (nlen < 1 || nlen > FASIM_MAX_DELETION_LENGTHS || !lengths) return fail(E, FASIM_E_ARG, "deletions: 1 to %d lengths, not %d", FASIM_MAX_DELETION_LENGTHS, nlen);
	for (int l = 0; l < nlen; l++) {
		if (lengths[l] < 1 || lengths[l] > FASIM_MAX_ALLELE - 1) return fail(E, FASIM_E_ARG, "deletions: length %d is outside [1, %d]", lengths[l], FASIM_MAX_ALLELE - 1);
		if (l > 0 && lengths[l] <= lengths[l - 1]) return fail(E, FASIM_E_ARG, "deletions: the lengths must ascend strictly (%d after %d)", lengths[l], lengths[l - 1]);
	}
	return FASIM_OK;
}

}  // namespace

int fasim_score_deletions(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_interval* ivs, int64_t nint, int32_t flank,
	const int32_t* lengths, int32_t nlen, const fasim_params* pp, fasim_del_score* out, fasim_deletion_stats* stats)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nint < 0 || (nint > 0 && (!ivs || !out))) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_variant_call(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, flank, pp, rs); if (rc) return rc;
	rc = check_lengths(E, lengths, nlen); if (rc) return rc;
	int64_t npos = 0;
	for (int64_t k = 0; k < nint; k++) {
		const fasim_interval& I = ivs[k];
		if (I.rec < 0 || I.rec >= nrec) return fail(E, FASIM_E_ARG, "interval %lld: record %d of %d", (long long)k, I.rec, nrec);
		if (I.start < 0 || I.end <= I.start || I.end > rec_len[I.rec])
			return fail(E, FASIM_E_ARG, "interval %lld: [%lld, %lld) is no stretch of record %d of %lld nt", (long long)k, (long long)I.start, (long long)I.end, I.rec, (long long)rec_len[I.rec]);
		if (I.end - I.start + 2 * (int64_t)flank > TOUCH_MAX_COLS)
			return fail(E, FASIM_E_ARG, "interval %lld: %lld positions and two flanks of %d are more than %d columns", (long long)k, (long long)(I.end - I.start), flank, TOUCH_MAX_COLS);
		npos += I.end - I.start;
	}
	const double t0 = now_s();
	const int dmax = lengths[nlen - 1];
	fasim_deletion_stats st;
	memset(&st, 0, sizeof st);
	st.intervals = nint; st.positions = npos;
	const char* host = rs.host(E);
	for (int q = 0; q < nq; q++) {
		fasim_del_score* row = out + (size_t)q * (size_t)npos * (size_t)nlen;
		int64_t at = 0;
		for (int64_t k = 0; k < nint; k++) for (int64_t x = ivs[k].start; x < ivs[k].end; x++) for (int l = 0; l < nlen; l++) {
			fasim_del_score& s = row[at++];
			memset(&s, 0, sizeof s);
			memset(s.enc, -1, sizeof s.enc);
			s.valid = x + lengths[l] < ivs[k].end;
			s.clean = s.valid && clean_run(host + rec_off[ivs[k].rec] + x, lengths[l] + 1);
			if (q == 0) st.deletions += s.valid;
		}
	}
	const std::vector<int> encs = enabled_encodings(*pp);
	const int nenc = (int)encs.size();
	if (st.deletions == 0 || nenc == 0) { st.total_s = now_s() - t0; if (stats) *stats = st; return FASIM_OK; }
	// one position of the longest interval must fit a launch: the bounds are not stretched for it
	int64_t longest = 0;
	for (int64_t k = 0; k < nint; k++) longest = std::max(longest, ivs[k].end - ivs[k].start);
	for (int q = 0; q < nq; q++) {
		const size_t state_rows = (size_t)touch_state_rows(rna_lens[q]);
		const int64_t cols = nenc * del_next(1, 0, longest, dmax), slots = cols + (int64_t)nenc * nlen;
		if ((size_t)cols * 4 * state_rows > MU_SNAP_BYTES || slots > MU_MAX_PROBS || (rna_lens[q] > TOUCH_LDS_ROWS && (size_t)slots * 6 * state_rows > MU_ROW_BYTES))
			return fail(E, FASIM_E_UNSUPPORTED, "deletions: query %d of %d nt under %d encodings with lengths up to %d needs %lld snapshot columns for one position, more than a launch holds: "
				"shorter lengths, fewer encodings or a shorter interval", q, rna_lens[q], nenc, dmax, (long long)cols);
	}
	HIPOK(hipSetDevice(E->device));
	try {
		for (int q = 0; q < nq; q++) {
			const int m = rna_lens[q];
			std::vector<uint8_t> qc((size_t)m);
			for (int i = 0; i < m; i++) qc[(size_t)i] = code2(rnas[q][i]);
			rc = upload(E, E->vr_q, qc.data(), qc.size()); if (rc) return rc;
			const bool rows_hbm = m > TOUCH_LDS_ROWS;
			const size_t state_rows = (size_t)touch_state_rows(m), row_bytes = 6 * state_rows, snap_bytes = 4 * state_rows;
			// what a launch holds: snapshot columns and problem slots (own-letter: one per snapshot column; ALT: nlen per position and encoding)
			const int64_t max_cols = std::max<int64_t>(1, (int64_t)(MU_SNAP_BYTES / snap_bytes));
			const int64_t max_probs = std::max<int64_t>(1, rows_hbm ? std::min<int64_t>(MU_MAX_PROBS, (int64_t)(MU_ROW_BYTES / row_bytes)) : MU_MAX_PROBS);
			fasim_del_score* row = out + (size_t)q * (size_t)npos * (size_t)nlen;
			int64_t it = 0, x = 0, gpos = 0;      // the next position: offset x of interval it, the call's position gpos
			while (it < nint) {
				std::vector<HapWindow> wins; std::vector<HapPiece> pieces; std::vector<int32_t> ends, first;
				std::vector<TouchProb> units; std::vector<DelGroup> groups; std::vector<uint8_t> letters;
				size_t tbytes = 0;
				int64_t lpos = 0, lcol = 0;      // positions and snapshot columns of the launch so far
				const int64_t gpos0 = gpos;
				while (it < nint) {
					const fasim_interval& I = ivs[it];
					const Context C = context_of(I, rec_len[I.rec], flank);
					const int n = (int)(C.hi - C.lo);
					const int64_t len = I.end - I.start;
					const size_t need = (size_t)nenc * (size_t)pad16(n);
					// the most positions whose columns and slots still fit (both grow with the positions taken)
					auto fits = [&](int64_t t) {
						const int64_t cols = lcol + nenc * del_next(t, x, len, dmax);
						return cols <= max_cols && cols + (lpos + t) * nenc * nlen <= max_probs;
					};
					int64_t take = 0;
					for (int64_t lo = 1, hi = len - x; lo <= hi; ) { const int64_t mid = (lo + hi) / 2; if (fits(mid)) { take = mid; lo = mid + 1; } else hi = mid - 1; }
					if (lpos > 0 && (take == 0 || tbytes + need > MU_TCODE_BYTES)) break;
					take = std::max<int64_t>(take, 1);      // (an empty launch holds one position: checked above)
					const int64_t next = del_next(take, x, len, dmax);
					HapPiece D; D.pad = 0; D.alt = 0; D.src = rec_off[I.rec] + C.lo;
					if (!rs.resident) { D.src = (int64_t)letters.size(); letters.insert(letters.end(), dna + rec_off[I.rec] + C.lo, dna + rec_off[I.rec] + C.hi); }
					HapWindow H; H.piece0 = (int64_t)pieces.size(); H.npiece = 1; H.pad = 0;
					pieces.push_back(D); ends.push_back(n);
					DelGroup G; G.unit0 = (int32_t)units.size(); G.pos0 = (int32_t)lpos; G.npos = (int32_t)take; G.next = (int32_t)next;
					const int a0 = (int)(I.start - C.lo + x), a1 = a0 + (int)next;
					const int edge_lo = C.lo > 0, edge_hi = C.hi < rec_len[I.rec];
					// the group's own-letter problems -- even encodings: the positions at which a deletion ends, odd: those at which one is
					// anchored -- and its deletions; the bounds are sums of 1 + n - r
					int64_t nown_even = 0, nown_odd = 0, ndel = 0, own_bound = 0, alt_bound_even = 0, alt_bound_odd = 0, own_bound_odd = 0;
					for (int64_t j = 0; j < next; j++) {
						bool used = false;
						for (int l = 0; l < nlen; l++) used |= j - lengths[l] >= 0 && j - lengths[l] < take;
						if (used) { nown_even++; own_bound += n - (a0 + j); }      // n - y, y the column
						if (j < take && j + lengths[0] < next) { nown_odd++; own_bound_odd += a0 + j + 1; }      // y = n - 1 - (a0 + j)
					}
					for (int64_t j = 0; j < take; j++) for (int l = 0; l < nlen; l++) if (j + lengths[l] < next) {
						ndel++;
						alt_bound_even += n - (a0 + j) - lengths[l];      // 1 + n - r, r = a + 1 + d
						alt_bound_odd += a0 + j + 1;                      // r = a + 1, a = n - 1 - (a0 + j)
					}
					for (int k = 0; k < nenc; k++) {
						TouchProb P; P.tbase = (int64_t)tbytes; P.n = n; P.win = (int32_t)wins.size(); P.enc = encs[(size_t)k];
						if (P.enc & 1) { P.v0 = n - a1; P.v1 = n - a0; P.edge = edge_hi | (edge_lo << 1); }
						else { P.v0 = a0; P.v1 = a1; P.edge = edge_lo | (edge_hi << 1); }
						first.push_back((int32_t)(lcol + (int64_t)k * next));
						units.push_back(P);
						tbytes += (size_t)pad16(n);
						st.prefix_cols += P.v1 - 1;
						st.cont_cols_bound += (P.enc & 1) ? own_bound_odd + alt_bound_odd : own_bound + alt_bound_even;
					}
					for (int k = 0; k < nenc; k++) st.own_problems += (encs[(size_t)k] & 1) ? nown_odd : nown_even;
					st.alt_problems += ndel * nenc;
					wins.push_back(H); groups.push_back(G);
					lpos += take; lcol += next * nenc; x += take;
					if (x == len) { it++; x = 0; }
				}
				gpos += lpos;
				const int nunit = (int)units.size(), ncol = (int)lcol;
				const int64_t nalt = lpos * nenc * nlen, nprob = ncol + nalt, nword = lpos * nlen;
				first.push_back(ncol);
				st.launches++; st.prefix_problems += nunit;
				if (E->vr_hwins.ensure(wins.size() * sizeof(HapWindow)) != hipSuccess || E->vr_pieces.ensure(pieces.size() * sizeof(HapPiece)) != hipSuccess ||
					E->vr_ends.ensure(ends.size() * sizeof(int32_t)) != hipSuccess || E->vr_probs.ensure((size_t)nunit * sizeof(TouchProb)) != hipSuccess ||
					E->mu_first.ensure(first.size() * sizeof(int32_t)) != hipSuccess || E->mu_groups.ensure(groups.size() * sizeof(DelGroup)) != hipSuccess ||
					E->vr_alt.ensure(1) != hipSuccess || E->vr_tcodes.ensure(tbytes) != hipSuccess || E->mu_snap.ensure((size_t)ncol * snap_bytes) != hipSuccess ||
					E->mu_pm.ensure((size_t)ncol * sizeof(uint32_t)) != hipSuccess ||
					E->vr_touch.ensure((size_t)nprob * sizeof(uint32_t)) != hipSuccess || E->mu_cols.ensure((size_t)nprob * sizeof(uint32_t)) != hipSuccess ||
					E->vr_out.ensure((size_t)nword * DEL_WORDS * sizeof(uint32_t)) != hipSuccess || (!rs.resident && E->vr_dna.ensure(letters.size() + 1) != hipSuccess) ||
					(rows_hbm && E->vr_rows.ensure((size_t)std::max<int64_t>(nprob, nunit) * row_bytes) != hipSuccess)) {
					(void)hipGetLastError();
					return fail(E, FASIM_E_NOMEM, "deletions: no device memory for a launch of %lld problems and %d snapshots", (long long)nprob, ncol);
				}
				HIPOK(hipMemcpyAsync(E->vr_hwins.p, wins.data(), wins.size() * sizeof(HapWindow), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_pieces.p, pieces.data(), pieces.size() * sizeof(HapPiece), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_ends.p, ends.data(), ends.size() * sizeof(int32_t), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_probs.p, units.data(), (size_t)nunit * sizeof(TouchProb), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->mu_first.p, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->mu_groups.p, groups.data(), groups.size() * sizeof(DelGroup), hipMemcpyHostToDevice, E->st));
				if (!rs.resident) HIPOK(hipMemcpyAsync(E->vr_dna.p, letters.data(), letters.size(), hipMemcpyHostToDevice, E->st));
				HapEncodeLaunch EL;
				EL.dna = rs.resident ? E->dna_res.as<uint8_t>() : E->vr_dna.as<uint8_t>(); EL.alts = E->vr_alt.as<uint8_t>(); EL.wins = E->vr_hwins.as<HapWindow>();
				EL.pieces = E->vr_pieces.as<HapPiece>(); EL.ends = E->vr_ends.as<int32_t>();
				EL.probs = E->vr_probs.as<TouchProb>(); EL.nprob = nunit; EL.enc_lut = E->enc_lut.as<uint8_t>(); EL.tcodes = E->vr_tcodes.as<uint8_t>();
				hipError_t he = launch_hap_encode(EL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "deletions (encode) launch failed: %s", hipGetErrorString(he));
				DelLaunch DL;
				memset(&DL, 0, sizeof DL);
				DL.tcodes = E->vr_tcodes.as<uint8_t>(); DL.qcodes = E->vr_q.as<uint8_t>(); DL.m = m; DL.units = E->vr_probs.as<TouchProb>();
				DL.first = E->mu_first.as<int32_t>(); DL.nunit = nunit; DL.ncol = ncol;
				DL.rows = rows_hbm ? E->vr_rows.as<uint16_t>() : nullptr; DL.snap = E->mu_snap.as<uint16_t>(); DL.pm = E->mu_pm.as<uint32_t>();
				DL.out = E->vr_touch.as<uint32_t>(); DL.cols = E->mu_cols.as<uint32_t>();
				DL.groups = E->mu_groups.as<DelGroup>(); DL.ngroup = (int32_t)groups.size(); DL.npos = (int32_t)lpos; DL.nenc = nenc; DL.nlen = nlen; DL.nalt = (int32_t)nalt;
				for (int l = 0; l < nlen; l++) DL.lengths[l] = (int16_t)lengths[l];
				for (int k = 0; k < nenc; k++) DL.enc[k] = (uint8_t)encs[(size_t)k];
				DL.words = E->vr_out.as<uint32_t>();
				KernelClock clock(E);
				clock.mark(0); he = launch_mut_prefix_pm(DL, E->st); clock.mark(1);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "deletions (prefix) launch failed: %s", hipGetErrorString(he));
				clock.mark(2); he = launch_mut_jump(DL, E->st); clock.mark(3);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "deletions (jump) launch failed: %s", hipGetErrorString(he));
				he = launch_mut_del_reduce(DL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "deletions (reduce) launch failed: %s", hipGetErrorString(he));
				std::vector<uint32_t> words((size_t)nword * DEL_WORDS);
				HIPOK(hipMemcpyAsync(words.data(), E->vr_out.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
				HIPOK(hipStreamSynchronize(E->st));
				st.prefix_s += clock.seconds(0, 1); st.cont_s += clock.seconds(2, 3);
				for (int64_t k = 0; k < nword; k++) {
					fasim_del_score& s = row[gpos0 * nlen + k];
					const uint32_t* w = &words[(size_t)k * DEL_WORDS];
					st.cont_cols += w[8];
					if (!s.valid || !w[9]) continue;
					for (int a = 0; a < 2; a++) {
						uint32_t top = 0;
						for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
							const uint32_t v = w[a * 4 + c];
							s.value[a][c] = (int32_t)(v >> 9);
							s.enc[a][c] = (v >> 9) ? (int8_t)(v & 0xff) : (int8_t)-1;
							top = std::max(top, v >> 8);
						}
						s.clipped[a] = (uint8_t)(top & 1);
					}
				}
			}
		}
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	st.total_s = now_s() - t0;
	if (stats) *stats = st;
	return FASIM_OK;
}

int fasim_deletions_tsv(const fasim_region* regions, const int64_t* offsets, int64_t n, const fasim_del_score* scores, const char* const* seqs,
	const int32_t* lengths, int32_t nlen, int32_t flank, const char* rna_name, char** text, int64_t* text_len)
{
	if (n < 0 || !rna_name || !text || !text_len || (n > 0 && (!regions || !offsets || !seqs))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	int rc = check_lengths(nullptr, lengths, nlen); if (rc) return rc;
	std::string o = "# fasim deletions lncRNA="; o += rna_name; o += " flank="; o += std::to_string(flank); o += " lengths=";
	for (int l = 0; l < nlen; l++) { if (l) o += ","; o += std::to_string(lengths[l]); }
	o += "\nline\tchrom\tpos\tid\tref\talt";
	for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "_ref\t"; o += c; o += "_alt"; }
	o += "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n";
	for (int64_t k = 0; k < n; k++) {
		const fasim_region& g = regions[k];
		if (!g.chrom || !g.name) return fail(nullptr, FASIM_E_ARG, "interval %lld lacks a string", (long long)k);
		const int64_t np = offsets[k + 1] - offsets[k];
		if (np == 0) continue;
		if (np != g.end - g.start || !scores || !seqs[k]) return fail(nullptr, FASIM_E_ARG, "interval %lld: %lld scores for %lld positions", (long long)k, (long long)np, (long long)(g.end - g.start));
		for (int64_t j = 0; j < np; j++) for (int l = 0; l < nlen; l++) {
			const fasim_del_score& s = scores[(offsets[k] + j) * nlen + l];
			const int d = lengths[l];
			if (!s.valid || !s.clean || j + d >= np) continue;
			int top[2] = { 0, 0 }, rule[2] = { -1, -1 };
			o += std::to_string(g.line); o += "\t"; o += g.chrom; o += "\t"; o += std::to_string(g.start + j + 1); o += "\t"; o += g.name;
			o += "\t"; o.append(seqs[k] + j, (size_t)d + 1); o += "\t"; o += seqs[k][j];
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
				o += "\t"; o += std::to_string(s.value[0][c]); o += "\t"; o += std::to_string(s.value[1][c]);
				for (int a = 0; a < 2; a++) if (s.value[a][c] > top[a]) { top[a] = s.value[a][c]; rule[a] = (s.enc[a][c] >= 0 && s.enc[a][c] < 48) ? enc_info(s.enc[a][c]).rule : -1; }
			}
			o += "\t"; o += std::to_string(top[0]); o += "\t"; o += std::to_string(top[1]); o += "\t"; o += std::to_string(top[1] - top[0]);
			for (int a = 0; a < 2; a++) { o += "\t"; o += (top[a] > 0 && rule[a] >= 0) ? std::to_string(rule[a]) : std::string("NA"); }
			// the bit of the larger of the two alleles' words; the maximum is taken on the doubled integer, so ties go to the bit
			o += "\t"; o += std::to_string(std::max(2 * top[0] + (s.clipped[0] & 1), 2 * top[1] + (s.clipped[1] & 1)) & 1); o += "\n";
		}
	}
	return text_out(o, text, text_len);
}
