// fasim-longtarget_amd/csrc/engine_variants.cpp -- fasim_score_variants: the triplex potential through variants (DESIGN.md section 19;
// kernels: haplotype.hip, variant.hip), and the table of `fasim --variants` (fasim_variants_tsv); fasim_score_variants_aligned: the same call with
// the alignment behind every score (section 21; kernel: variant_path.hip), its projection to the reference and its table;
// fasim_score_haplotypes: every entry on the two haplotypes of a sample (section 25; kernel: haplotype.hip), its planner and its table.
//
// What is scored is a unit: two allele windows that share their sides -- the left pieces, the REF letters in the record or the ALT
// string, the right pieces -- and a window under an enabled encoding is a problem.  A variant of section 19 is the unit whose sides are
// the record stretches of its flanks; an (entry, haplotype) of section 25 is the unit whose sides the planner walked.  Per query the
// units are cut into chunks by a fixed bound on buffer bytes, by run_units alone; a chunk is: the windows as pieces (and, for a
// streamed record, their letters) and the ALT letters up, k_hap_encode, k_touch, k_touch_reduce, nine words per unit back.
// Everything runs on the engine's own stream and in buffers of its own (vr_*): the engine's query, its scan buffers and its workers
// are not touched.
// The aligned call adds per chunk, after the nine words are back: the slots with a value become path items over the target codes
// that are still in vr_tcodes, k_touch_path in launches of at most 512 MB of direction bytes, cells and CIGARs back, convert_triplex
// (on the host while the next launch's kernel runs).
#include <climits>

#include "engine.h"

namespace {

constexpr size_t VR_TCODE_BYTES = (size_t)16 << 20;      // target codes of a chunk
constexpr size_t VR_ROW_BYTES = (size_t)256 << 20;       // HBM row state of a chunk (queries above TOUCH_LDS_ROWS)
constexpr int64_t VR_MAX_PROBS = 1 << 20;                // problems of a chunk

inline int pad16(int n) { return (n + 15) & ~15; }

constexpr int64_t VR_DIR_BYTES = (int64_t)512 << 20;      // direction bytes of a path launch
constexpr int64_t VR_CIG_WORDS = (int64_t)1 << 26;        // CIGAR words of a path launch

// the window of a variant: [lo, hi) of its record
inline void window_of(const fasim_variant& x, int64_t len, int32_t flank, int64_t& lo, int64_t& hi)
{
	lo = std::max<int64_t>(0, x.pos - flank); hi = std::min<int64_t>(len, x.pos + x.ref_len + flank);
}

inline void blank_score(fasim_variant_score& s)
{
	memset(&s, 0, sizeof s);
	for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) s.enc[a][c] = -1;
}

}  // namespace

// the refusals of a call that scores variants, before its entries are looked at
int check_variant_call(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna, const int64_t* rec_off,
	const int64_t* rec_len, int32_t nrec, int32_t flank, const fasim_params* pp, RecordSet& rs)
{
	if (nq < 1 || !rnas || !rna_lens || !pp) return fail(E, FASIM_E_ARG, "bad arguments");
	int rc = record_set_open(E, dna, rec_off, rec_len, nrec, false, rs); if (rc) return rc;
	for (int32_t q = 0; q < nq; q++) {
		if (!rnas[q] || rna_lens[q] <= 0) return fail(E, FASIM_E_ARG, "empty query %d", q);
		if (rna_lens[q] > FASIM_MAX_QUERY) return fail(E, FASIM_E_UNSUPPORTED, "query %d has %d nt: the limit is %d", q, rna_lens[q], FASIM_MAX_QUERY);
	}
	if (pp->classicSim) return fail(E, FASIM_E_UNSUPPORTED, "variants are scored with the fastSIM scoring only: not with classicSim (-F)");
	if (flank < 0 || flank > FASIM_MAX_FLANK) return fail(E, FASIM_E_ARG, "flank %d lies outside [0, %d]", flank, FASIM_MAX_FLANK);
	return record_set_bounds(E, rs);
}

namespace {

// the refusals for the entries themselves
int check_variant_entries(fasim_engine* E, const fasim_variant* vars, int64_t nvar, const int64_t* rec_len, int32_t nrec)
{
	for (int64_t v = 0; v < nvar; v++) {
		const fasim_variant& x = vars[v];
		if (x.alt_len < 0) continue;
		if (x.ref_len < 1) return fail(E, FASIM_E_ARG, "variant %lld: ref_len %d < 1", (long long)v, x.ref_len);
		if (x.ref_len > FASIM_MAX_ALLELE || x.alt_len < 1 || x.alt_len > FASIM_MAX_ALLELE || !x.alt)
			return fail(E, FASIM_E_ARG, "variant %lld: an allele has 1 to %d letters (REF %d, ALT %d)", (long long)v, FASIM_MAX_ALLELE, x.ref_len, x.alt_len);
		if (x.rec < 0 || x.rec >= nrec) return fail(E, FASIM_E_ARG, "variant %lld: record %d of %d", (long long)v, x.rec, nrec);
		if (x.pos < 0 || x.pos > rec_len[x.rec] - x.ref_len)
			return fail(E, FASIM_E_ARG, "variant %lld: [%lld, %lld) lies outside record %d of %lld nt", (long long)v, (long long)x.pos,
				(long long)(x.pos + x.ref_len), x.rec, (long long)rec_len[x.rec]);
	}
	return FASIM_OK;
}

// ---- scoring units and their chunks --------------------------------------------------------------------------------------------------
struct HPiece { int64_t src; int32_t len; int64_t ent; };      // ent < 0: record letters [src, src + len); else letters [src, src + len) of entry ent's ALT
struct HapSides { std::vector<HPiece> left, right; int32_t applied = 0; bool edge_lo = false, edge_hi = false; };
// One unit: the focus entry v between its sides; `out` takes its score
struct ScoreUnit { int64_t v; const HapSides* sides; fasim_variant_score* out; };

inline int32_t pieces_len(const std::vector<HPiece>& p) { int32_t n = 0; for (const HPiece& q : p) n += q.len; return n; }

// the sides of a variant of section 19: the record stretches of its window; a side of no letters is no piece
void plain_sides(const fasim_variant& x, int64_t len, int32_t flank, HapSides& S)
{
	int64_t lo, hi;
	window_of(x, len, flank, lo, hi);
	S.left.clear(); S.right.clear();
	if (lo < x.pos) S.left.push_back({ lo, (int32_t)(x.pos - lo), -1 });
	if (x.pos + x.ref_len < hi) S.right.push_back({ x.pos + x.ref_len, (int32_t)(hi - x.pos - x.ref_len), -1 });
	S.edge_lo = lo > 0; S.edge_hi = hi < len;      // cut by the flank, not by the record's end
}

// What the chunks of a call need of it: `who` is the call's word in the error texts; the query is the one open_query uploaded last;
// nprobs and cells count over the whole call
struct UnitRun {
	fasim_engine* E; const char* who; const char* dna; bool resident; const int64_t* rec_off; const fasim_variant* vars; const std::vector<int>* encs;
	int m = 0; bool rows_hbm = false; size_t row_bytes = 0;      // row_bytes: of one problem
	int64_t nprobs = 0, cells = 0;
};

int open_query(UnitRun& R, const char* rna, int m)
{
	std::vector<uint8_t> qc((size_t)m);
	for (int i = 0; i < m; i++) qc[(size_t)i] = code2(rna[i]);
	R.m = m; R.rows_hbm = m > TOUCH_LDS_ROWS; R.row_bytes = (size_t)6 * (size_t)touch_state_rows(m);
	return upload(R.E, R.E->vr_q, qc.data(), qc.size());
}

// The units unit_at(0 .. nunit) against the open query, in chunks.  After a chunk's scores are in place and while its problems -- in
// (unit, allele, encoding) order -- and their target codes are still on the device: chunk_done(first unit, units, problems)
template <class UnitAt, class ChunkDone>
int run_units(UnitRun& R, size_t nunit, UnitAt unit_at, ChunkDone chunk_done)
{
	fasim_engine* E = R.E;
	const std::vector<int>& encs = *R.encs;
	const int nenc = (int)encs.size(), m = R.m;
	std::vector<HapPiece> dl, dr;
	for (size_t u0 = 0; u0 < nunit; ) {
		std::vector<HapWindow> wins;
		std::vector<HapPiece> pieces;
		std::vector<int32_t> ends;
		std::vector<TouchProb> probs;
		std::vector<uint8_t> alts, letters;
		std::vector<fasim_variant_score*> outs;
		size_t tbytes = 0, u1 = u0;
		for (; u1 < nunit; u1++) {
			const ScoreUnit U = unit_at(u1);
			const fasim_variant& x = R.vars[U.v];
			const HapSides& W = *U.sides;
			const int pre = pieces_len(W.left), post = pieces_len(W.right);
			const int n_al[2] = { pre + x.ref_len + post, pre + x.alt_len + post };
			const size_t need = (size_t)nenc * (size_t)(pad16(n_al[0]) + pad16(n_al[1]));
			if (u1 > u0 && (tbytes + need > VR_TCODE_BYTES || (int64_t)probs.size() + 2 * nenc > VR_MAX_PROBS ||
				(R.rows_hbm && (probs.size() + 2 * (size_t)nenc) * R.row_bytes > VR_ROW_BYTES))) break;
			// the unit's pieces for the device: record letters in the resident buffer or staged for this chunk, ALT letters uploaded
			auto device_piece = [&](const HPiece& p) {
				HapPiece D; D.pad = 0;
				if (p.ent < 0) {
					D.alt = 0; D.src = R.rec_off[x.rec] + p.src;
					if (!R.resident) { D.src = (int64_t)letters.size(); letters.insert(letters.end(), R.dna + R.rec_off[x.rec] + p.src, R.dna + R.rec_off[x.rec] + p.src + p.len); }
				} else {
					D.alt = 1; D.src = (int64_t)alts.size();
					alts.insert(alts.end(), R.vars[p.ent].alt + p.src, R.vars[p.ent].alt + p.src + p.len);
				}
				return D;
			};
			// (the sides go up once for both alleles: of a streamed record every letter of the windows is staged once)
			dl.clear(); dr.clear();
			for (const HPiece& p : W.left) dl.push_back(device_piece(p));
			for (const HPiece& p : W.right) dr.push_back(device_piece(p));
			const HPiece focus[2] = { { x.pos, x.ref_len, -1 }, { 0, x.alt_len, U.v } };
			const int edge_lo = W.edge_lo, edge_hi = W.edge_hi;
			for (int al = 0; al < 2; al++) {
				HapWindow H; H.piece0 = (int64_t)pieces.size(); H.npiece = (int32_t)(dl.size() + 1 + dr.size()); H.pad = 0;
				int32_t run = 0;
				for (size_t k = 0; k < dl.size(); k++) { pieces.push_back(dl[k]); run += W.left[k].len; ends.push_back(run); }
				pieces.push_back(device_piece(focus[al])); run += focus[al].len; ends.push_back(run);
				for (size_t k = 0; k < dr.size(); k++) { pieces.push_back(dr[k]); run += W.right[k].len; ends.push_back(run); }
				const int n = n_al[al], v0 = pre, v1 = pre + focus[al].len;
				if (run != n || n > TOUCH_MAX_COLS) return fail(E, FASIM_E_ARG, "%s: a window of %d letters in pieces of %d", R.who, n, run);
				for (int k = 0; k < nenc; k++) {
					const int enc = encs[(size_t)k];
					TouchProb P; P.tbase = (int64_t)tbytes; P.n = n; P.win = (int32_t)wins.size(); P.enc = enc;
					if (enc & 1) { P.v0 = n - v1; P.v1 = n - v0; P.edge = edge_hi | (edge_lo << 1); }
					else { P.v0 = v0; P.v1 = v1; P.edge = edge_lo | (edge_hi << 1); }
					probs.push_back(P);
					tbytes += (size_t)pad16(n);
					R.cells += (int64_t)m * n;
				}
				wins.push_back(H);
			}
			outs.push_back(U.out);
		}
		const int np = (int)probs.size(), nu = (int)(u1 - u0);
		R.nprobs += np;
		if (alts.empty()) alts.push_back(0);
		if (E->vr_hwins.ensure(wins.size() * sizeof(HapWindow)) != hipSuccess || E->vr_pieces.ensure(pieces.size() * sizeof(HapPiece)) != hipSuccess ||
			E->vr_ends.ensure(ends.size() * sizeof(int32_t)) != hipSuccess || E->vr_probs.ensure((size_t)np * sizeof(TouchProb)) != hipSuccess ||
			E->vr_alt.ensure(alts.size()) != hipSuccess || E->vr_tcodes.ensure(tbytes) != hipSuccess || E->vr_touch.ensure((size_t)np * sizeof(uint32_t)) != hipSuccess ||
			E->vr_out.ensure((size_t)nu * 9 * sizeof(uint32_t)) != hipSuccess || (!R.resident && E->vr_dna.ensure(letters.size() + 1) != hipSuccess) ||
			(R.rows_hbm && E->vr_rows.ensure((size_t)np * R.row_bytes) != hipSuccess)) {
			(void)hipGetLastError();
			return fail(E, FASIM_E_NOMEM, "%s: no device memory for a chunk of %d problems", R.who, np);
		}
		HIPOK(hipMemcpyAsync(E->vr_hwins.p, wins.data(), wins.size() * sizeof(HapWindow), hipMemcpyHostToDevice, E->st));
		HIPOK(hipMemcpyAsync(E->vr_pieces.p, pieces.data(), pieces.size() * sizeof(HapPiece), hipMemcpyHostToDevice, E->st));
		HIPOK(hipMemcpyAsync(E->vr_ends.p, ends.data(), ends.size() * sizeof(int32_t), hipMemcpyHostToDevice, E->st));
		HIPOK(hipMemcpyAsync(E->vr_probs.p, probs.data(), (size_t)np * sizeof(TouchProb), hipMemcpyHostToDevice, E->st));
		HIPOK(hipMemcpyAsync(E->vr_alt.p, alts.data(), alts.size(), hipMemcpyHostToDevice, E->st));
		if (!R.resident && !letters.empty()) HIPOK(hipMemcpyAsync(E->vr_dna.p, letters.data(), letters.size(), hipMemcpyHostToDevice, E->st));
		HapEncodeLaunch EL;
		EL.dna = R.resident ? E->dna_res.as<uint8_t>() : E->vr_dna.as<uint8_t>(); EL.alts = E->vr_alt.as<uint8_t>(); EL.wins = E->vr_hwins.as<HapWindow>();
		EL.pieces = E->vr_pieces.as<HapPiece>(); EL.ends = E->vr_ends.as<int32_t>();
		EL.probs = E->vr_probs.as<TouchProb>(); EL.nprob = np; EL.enc_lut = E->enc_lut.as<uint8_t>(); EL.tcodes = E->vr_tcodes.as<uint8_t>();
		hipError_t he = launch_hap_encode(EL, E->st);
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "%s (encode) launch failed: %s", R.who, hipGetErrorString(he));
		TouchLaunch TL;
		TL.tcodes = E->vr_tcodes.as<uint8_t>(); TL.qcodes = E->vr_q.as<uint8_t>(); TL.m = m; TL.probs = E->vr_probs.as<TouchProb>(); TL.nprob = np;
		TL.rows = R.rows_hbm ? E->vr_rows.as<uint16_t>() : nullptr; TL.out = E->vr_touch.as<uint32_t>();
		{ TimedScope ts(E, 4); he = launch_touch(TL, E->st); }
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "%s (touch) launch failed: %s", R.who, hipGetErrorString(he));
		TouchReduceLaunch RL;
		RL.touch = E->vr_touch.as<uint32_t>(); RL.nvar = nu; RL.nenc = nenc; RL.out = E->vr_out.as<uint32_t>();
		memset(RL.enc, 0, sizeof RL.enc);
		for (int k = 0; k < nenc; k++) RL.enc[k] = (uint8_t)encs[(size_t)k];
		he = launch_touch_reduce(RL, E->st);
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "%s (reduce) launch failed: %s", R.who, hipGetErrorString(he));
		std::vector<uint32_t> words((size_t)nu * 9);
		HIPOK(hipMemcpyAsync(words.data(), E->vr_out.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
		HIPOK(hipStreamSynchronize(E->st));
		drain_timed(E);
		for (int k = 0; k < nu; k++) {
			fasim_variant_score& s = *outs[(size_t)k];
			for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
				const uint32_t w = words[(size_t)k * 9 + (size_t)a * 4 + (size_t)c];
				s.value[a][c] = (int32_t)(w >> 9);
				s.enc[a][c] = (w >> 9) ? (int32_t)(w & 0xff) : -1;
			}
			s.flags = (int32_t)(words[(size_t)k * 9 + 8] & 1);
		}
		const int rc = chunk_done(u0, nu, probs); if (rc) return rc;
		u0 = u1;
	}
	return FASIM_OK;
}

// What the path phase of a chunk needs of its call
struct PathCtx {
	fasim_engine* E; std::string rna; int m; std::vector<int> encs; const char* host; const int64_t* rec_off; const int64_t* rec_len;
	const fasim_variant* vars; int32_t flank; fasim_params pc; bool rows_hbm; size_t row_bytes;
};

// The hits of the chunk's variants todo[0 .. nv): probs are the chunk's problems in (variant, allele, encoding) order, still on the
// device with their target codes; scores the query's row of the call's results; H the query's 8 * nvar hits
int trace_chunk(const PathCtx& C, const std::vector<TouchProb>& probs, const int64_t* todo, int nv, const fasim_variant_score* scores,
	std::vector<HitOut>& H)
{
	fasim_engine* E = C.E;
	const int nenc = (int)C.encs.size(), m = C.m;
	const int64_t rows = touch_state_rows(m);
	struct Want { size_t slot; int64_t v; int al, enc, value; };
	std::vector<TouchPathItem> items;
	std::vector<Want> wants;
	for (int k = 0; k < nv; k++) {
		const int64_t v = todo[k];
		const fasim_variant_score& s = scores[v];
		for (int al = 0; al < 2; al++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			if (s.value[al][c] <= 0) continue;
			const size_t slot = ((size_t)v * 2 + (size_t)al) * 4 + (size_t)c;
			HitOut& h = H[slot];
			h.empty = false; h.t.enc = s.enc[al][c];
			const auto it = std::find(C.encs.begin(), C.encs.end(), s.enc[al][c]);
			if (it == C.encs.end()) continue;
			const int prob = (k * 2 + al) * nenc + (int)(it - C.encs.begin());
			const TouchProb& P = probs[(size_t)prob];
			if ((int64_t)m * P.n > TOUCH_PATH_MAX_CELLS) continue;      // left unaligned
			TouchPathItem I; I.dir_off = 0; I.prob = prob; I.value = s.value[al][c]; I.cig_off = 0; I.cig_cap = 2 * P.n + 1;
			items.push_back(I);
			wants.push_back({ slot, v, al, s.enc[al][c], s.value[al][c] });
		}
	}
	std::string alt_win;
	// the host's half of a launch: cells and CIGARs into hits.  It runs while the next launch's kernel does
	struct Done { size_t a = 0; int ni = 0; std::vector<TouchPathOut> outs; std::vector<uint32_t> cig; } prev;
	auto finish = [&](const Done& D) {
		const size_t a = D.a; const int ni = D.ni;
		const std::vector<TouchPathOut>& outs = D.outs; const std::vector<uint32_t>& cig = D.cig;
		for (int k = 0; k < ni; k++) {
			const TouchPathItem& I = items[a + (size_t)k];
			const Want& w = wants[a + (size_t)k];
			const TouchPathOut& o = outs[(size_t)k];
			const int n = probs[(size_t)I.prob].n;
			HitOut& h = H[w.slot];
			h.i0 = o.i0; h.i1 = o.i1; h.j0 = o.j0; h.j1 = o.j1;
			if (o.cigar_len < 1 || o.cigar_len > I.cig_cap || o.i0 < 0 || o.j0 < 0 || o.i0 > o.i1 || o.j0 > o.j1 || o.i1 >= m || o.j1 >= n) continue;
			// the window's letters: the record's own, or the ALT window assembled here
			const fasim_variant& x = C.vars[w.v];
			int64_t lo, hi;
			window_of(x, C.rec_len[x.rec], C.flank, lo, hi);
			const char* seg = C.host + C.rec_off[x.rec] + lo;
			if (w.al) {
				alt_win.assign(seg, (size_t)(x.pos - lo));
				alt_win.append(x.alt, (size_t)x.alt_len);
				alt_win.append(C.host + C.rec_off[x.rec] + x.pos + x.ref_len, (size_t)(hi - x.pos - x.ref_len));
				seg = alt_win.data();
			}
			path_hit(h, cig.data() + I.cig_off, o.cigar_len, w.value, C.rna, seg, n, w.enc, (long)lo, C.pc, (int)w.v);
		}
	};
	for (size_t a = 0; a < items.size(); ) {
		const LaunchCut cut = cut_launch(items, a, VR_DIR_BYTES, VR_CIG_WORDS, [&](const TouchPathItem& I) { return std::pair<int64_t, int64_t>(rows, probs[(size_t)I.prob].n); });
		const int ni = (int)(cut.end - a);
		if (E->vr_items.ensure((size_t)ni * sizeof(TouchPathItem)) != hipSuccess || E->vr_dirs.ensure((size_t)cut.dir_total) != hipSuccess ||
			E->vr_cigar.ensure((size_t)cut.cig_total * sizeof(uint32_t)) != hipSuccess || E->vr_paths.ensure((size_t)ni * sizeof(TouchPathOut)) != hipSuccess ||
			(C.rows_hbm && E->vr_rows.ensure((size_t)ni * C.row_bytes) != hipSuccess)) {
			(void)hipGetLastError();
			return fail(E, FASIM_E_NOMEM, "variant hits: no device memory for the direction bytes of %d paths (%lld bytes)", ni, (long long)cut.dir_total);
		}
		HIPOK(hipMemcpyAsync(E->vr_items.p, items.data() + a, (size_t)ni * sizeof(TouchPathItem), hipMemcpyHostToDevice, E->st));
		TouchPathLaunch PL;
		PL.tcodes = E->vr_tcodes.as<uint8_t>(); PL.qcodes = E->vr_q.as<uint8_t>(); PL.m = m; PL.probs = E->vr_probs.as<TouchProb>();
		PL.items = E->vr_items.as<TouchPathItem>(); PL.nitem = ni; PL.rows = C.rows_hbm ? E->vr_rows.as<uint16_t>() : nullptr;
		PL.dirs = E->vr_dirs.as<uint8_t>(); PL.cigar = E->vr_cigar.as<uint32_t>(); PL.out = E->vr_paths.as<TouchPathOut>();
		hipError_t he;
		{ TimedScope ts(E, 4); he = launch_touch_path(PL, E->st); }
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "variant hits (path) launch failed: %s", hipGetErrorString(he));
		if (prev.ni) finish(prev);      // (before the copies back: they wait for the kernel)
		Done cur; cur.a = a; cur.ni = ni; cur.outs.resize((size_t)ni); cur.cig.resize((size_t)cut.cig_total);
		HIPOK(hipMemcpyAsync(cur.outs.data(), E->vr_paths.p, (size_t)ni * sizeof(TouchPathOut), hipMemcpyDeviceToHost, E->st));
		HIPOK(hipMemcpyAsync(cur.cig.data(), E->vr_cigar.p, (size_t)cut.cig_total * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
		HIPOK(hipStreamSynchronize(E->st));
		drain_timed(E);
		prev = std::move(cur);
		a = cut.end;
	}
	if (prev.ni) finish(prev);
	return FASIM_OK;
}

// fasim_score_variants; with `hits` (and `windows`) fasim_score_variants_aligned
int score_variants_impl(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_variant* vars, int64_t nvar, int32_t flank,
	const fasim_params* pp, fasim_variant_score* out, fasim_variant_stats* stats, fasim_variant_window* windows, fasim_site_hits** hits)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nvar < 0 || (nvar > 0 && (!vars || !out))) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_variant_call(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, flank, pp, rs); if (rc) return rc;
	rc = check_variant_entries(E, vars, nvar, rec_len, nrec); if (rc) return rc;
	const double t0 = now_s();
	if (stats) memset(stats, 0, sizeof *stats);
	if (hits) {
		for (int64_t v = 0; v < nvar; v++) {
			const fasim_variant& x = vars[v];
			memset(&windows[v], 0, sizeof windows[v]);
			if (x.alt_len < 0 || x.rec < 0 || x.rec >= nrec || x.pos < 0 || x.pos > rec_len[x.rec] - x.ref_len) continue;
			int64_t lo, hi;
			window_of(x, rec_len[x.rec], flank, lo, hi);
			windows[v].pre = (int32_t)(x.pos - lo); windows[v].post = (int32_t)(hi - x.pos - x.ref_len);
			windows[v].edge = (lo > 0 ? 1 : 0) | (hi < rec_len[x.rec] ? 2 : 0);
		}
	}
	// the hits of a query before any path is traced: every slot empty
	auto blank_hits = [&](std::vector<HitOut>& H) {
		H.assign((size_t)nvar * 8, HitOut());
		for (size_t k = 0; k < H.size(); k++) { hit_clear(H[k], -1); H[k].t.seg = (int)(k / 8); H[k].empty = true; }
	};
	for (int64_t k = 0; k < (int64_t)nq * nvar; k++) blank_score(out[k]);
	const std::vector<int> encs = enabled_encodings(*pp);
	const int nenc = (int)encs.size();
	std::vector<int64_t> todo;                  // the variants that are scored
	for (int64_t v = 0; v < nvar; v++) if (vars[v].alt_len >= 0) todo.push_back(v);
	if (todo.empty() || nenc == 0) {
		if (hits) {
			try {
				std::vector<HitOut> H;
				blank_hits(H);
				for (int q = 0; q < nq; q++) if (!(hits[q] = pack_hits(H))) return fail(E, FASIM_E_NOMEM, "out of memory");
			} catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
		}
		if (stats) stats->total_s = now_s() - t0;
		return FASIM_OK;
	}
	HIPOK(hipSetDevice(E->device));
	const double ms0 = E->kernel_ms[4];
	UnitRun R{ E, "variants", dna, rs.resident, rec_off, vars, &encs };
	try {
		for (int q = 0; q < nq; q++) {
			rc = open_query(R, rnas[q], rna_lens[q]); if (rc) return rc;
			fasim_variant_score* row = out + (size_t)q * (size_t)nvar;
			std::vector<HitOut> H;
			PathCtx PC;
			if (hits) {
				blank_hits(H);
				PC.E = E; PC.rna.assign(rnas[q], rnas[q] + R.m); PC.m = R.m; PC.encs = encs; PC.host = rs.host(E); PC.rec_off = rec_off; PC.rec_len = rec_len;
				PC.vars = vars; PC.flank = flank; PC.pc = *pp; PC.pc.ntMin = 1; PC.pc.ntMax = INT_MAX; PC.rows_hbm = R.rows_hbm; PC.row_bytes = R.row_bytes;
			}
			HapSides W;      // of the unit asked for last
			rc = run_units(R, todo.size(),
				[&](size_t k) { const int64_t v = todo[k]; plain_sides(vars[v], rec_len[vars[v].rec], flank, W); return ScoreUnit{ v, &W, &row[v] }; },
				[&](size_t u0, int nu, const std::vector<TouchProb>& probs) { return hits ? trace_chunk(PC, probs, todo.data() + u0, nu, row, H) : FASIM_OK; });
			if (rc) return rc;
			if (hits && !(hits[q] = pack_hits(H))) return fail(E, FASIM_E_NOMEM, "out of memory");
		}
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (stats) { stats->problems = R.nprobs; stats->cells = R.cells; stats->kernel_s = (E->kernel_ms[4] - ms0) * 1e-3; stats->total_s = now_s() - t0; }
	return FASIM_OK;
}

}  // namespace

int fasim_score_variants(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_variant* vars, int64_t nvar, int32_t flank,
	const fasim_params* pp, fasim_variant_score* out, fasim_variant_stats* stats)
{
	return score_variants_impl(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, vars, nvar, flank, pp, out, stats, nullptr, nullptr);
}

int fasim_score_variants_aligned(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_variant* vars, int64_t nvar, int32_t flank,
	const fasim_params* pp, fasim_variant_score* out, fasim_variant_stats* stats, fasim_variant_window* windows, fasim_site_hits** hits)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!hits || (nvar > 0 && !windows)) return fail(E, FASIM_E_ARG, "bad arguments");
	for (int32_t q = 0; q < nq; q++) hits[q] = nullptr;
	const int rc = score_variants_impl(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, vars, nvar, flank, pp, out, stats, windows, hits);
	if (rc) {
		(void)hipStreamSynchronize(E->st);
		for (int32_t q = 0; q < nq; q++) { site_hits_free(hits[q]); hits[q] = nullptr; }
	}
	return rc;
}

int fasim_variant_hit_span(const fasim_variant* v, const fasim_variant_window* w, int32_t allele, int32_t enc, int32_t j0, int32_t j1,
	int64_t* start, int64_t* end, int32_t* clipped)
{
	if (!v || !w || !start || !end || allele < 0 || allele > 1 || enc < 0 || enc >= 48) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	const int64_t pre = w->pre, alen = allele ? v->alt_len : v->ref_len, n = pre + alen + w->post;
	if (alen < 1 || pre < 0 || w->post < 0 || j0 < 0 || j0 > j1 || j1 >= n) return fail(nullptr, FASIM_E_ARG, "columns [%d, %d] lie outside the window of %lld letters", j0, j1, (long long)n);
	const int64_t w0 = (enc & 1) ? n - 1 - j1 : j0, w1 = (enc & 1) ? n - 1 - j0 : j1;
	const int64_t a = v->pos;
	*start = w0 < pre ? a - pre + w0 : (w0 < pre + alen ? a : a + v->ref_len + (w0 - pre - alen));
	*end = w1 < pre ? a - pre + w1 + 1 : (w1 < pre + alen ? a + v->ref_len : a + v->ref_len + (w1 - pre - alen) + 1);
	if (clipped) {
		const int first = (enc & 1) ? (w->edge >> 1) & 1 : w->edge & 1, last = (enc & 1) ? w->edge & 1 : (w->edge >> 1) & 1;      // the unit's ends
		*clipped = ((j0 == 0 && first) || (j1 == n - 1 && last)) ? 1 : 0;
	}
	return FASIM_OK;
}

int fasim_variant_hits_tsv(const fasim_variant* vars, const fasim_variant_score* scores, const fasim_variant_window* windows,
	const fasim_site_hits* hits, int64_t nvar, int32_t flank, const char* rna_name, const uint8_t* matched, char** text, int64_t* text_len)
{
	if (nvar < 0 || !rna_name || !text || !text_len || !hits || hits->n != 8 * nvar || (nvar > 0 && (!vars || !scores || !windows)))
		return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "# fasim variant hits lncRNA="; o += rna_name; o += " flank="; o += std::to_string(flank); o += "\n";
	o += "line\tchrom\tpos\tid\tref\talt\tallele\tclass\tvalue\trule\tstrand\ttts_start\ttts_end\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tclipped\tTFO\tTTS\n";
	char b[128];
	for (int64_t k = 0; k < nvar; k++) {
		const fasim_variant& x = vars[k];
		if (!x.chrom || !x.id || !x.ref || !x.alt) return fail(nullptr, FASIM_E_ARG, "variant %lld lacks a string", (long long)k);
		if ((matched && !matched[k]) || x.alt_len < 0) continue;
		const fasim_variant_score& s = scores[k];
		for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			if (s.value[a][c] <= 0) continue;
			const int64_t i = (k * 2 + a) * 4 + c;
			const fasim_triplex& t = hits->t[i];
			const int enc = s.enc[a][c];
			o += std::to_string(x.line); o += "\t"; o += x.chrom; o += "\t"; o += std::to_string(x.pos + 1); o += "\t"; o += x.id; o += "\t"; o += x.ref; o += "\t"; o += x.alt;
			int n = snprintf(b, sizeof b, "\t%s\t%s\t%d\t", a ? "alt" : "ref", CLASS_NAMES[c], s.value[a][c]);
			o.append(b, (size_t)n);
			o += (enc >= 0 && enc < 48) ? std::to_string(enc_info(enc).rule) : std::string("NA");
			o += (c == 0 || c == 3) ? "\t+" : "\t-";
			int64_t st = 0, en = 0; int32_t clip = 0;
			const bool al = hits->cigar_len[i] > 0 && enc >= 0 && enc < 48 &&
				fasim_variant_hit_span(&x, &windows[k], a, enc, hits->t_begin[i], hits->t_end[i], &st, &en, &clip) == FASIM_OK;
			if (!al) { o += "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"; continue; }
			n = snprintf(b, sizeof b, "\t%lld\t%lld\t%d\t%d\t%d\t%g\t%g\t", (long long)st, (long long)en, t.stari, t.endi, t.nt, (double)t.identity, (double)t.tri_score);
			o.append(b, (size_t)n);
			for (int32_t j = 0; j < hits->cigar_len[i]; j++) {
				const uint32_t w = hits->cigar[hits->cigar_off[i] + j];
				n = snprintf(b, sizeof b, "%u%c", w >> 4, "MID"[(w & 15) < 3 ? (w & 15) : 0]);
				o.append(b, (size_t)n);
			}
			o += clip ? "\t1\t" : "\t0\t"; o += hits->pool + t.tfo_off; o += "\t"; o += hits->pool + t.tts_off; o += "\n";
		}
	}
	return text_out(o, text, text_len);
}

int fasim_variants_tsv(const fasim_variant* vars, const fasim_variant_score* scores, int64_t nvar, int32_t flank, const char* rna_name,
	const uint8_t* matched, char** text, int64_t* text_len)
{
	if (nvar < 0 || !rna_name || !text || !text_len || (nvar > 0 && (!vars || !scores))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "# fasim variants lncRNA="; o += rna_name; o += " flank="; o += std::to_string(flank); o += "\n";
	o += "line\tchrom\tpos\tid\tref\talt";
	for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "_ref\t"; o += c; o += "_alt"; }
	o += "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n";
	for (int64_t k = 0; k < nvar; k++) {
		const fasim_variant& x = vars[k];
		if (!x.chrom || !x.id || !x.ref || !x.alt) return fail(nullptr, FASIM_E_ARG, "variant %lld lacks a string", (long long)k);
		o += std::to_string(x.line); o += "\t"; o += x.chrom; o += "\t"; o += std::to_string(x.pos + 1); o += "\t"; o += x.id; o += "\t"; o += x.ref; o += "\t"; o += x.alt;
		if ((matched && !matched[k]) || x.alt_len < 0) { for (int c = 0; c < 2 * FASIM_TRACK_CLASSES + 6; c++) o += "\tNA"; o += "\n"; continue; }
		const fasim_variant_score& s = scores[k];
		int top[2] = { 0, 0 }, rule[2] = { -1, -1 };
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			o += "\t"; o += std::to_string(s.value[0][c]); o += "\t"; o += std::to_string(s.value[1][c]);
			for (int a = 0; a < 2; a++) if (s.value[a][c] > top[a]) { top[a] = s.value[a][c]; rule[a] = (s.enc[a][c] >= 0 && s.enc[a][c] < 48) ? enc_info(s.enc[a][c]).rule : -1; }
		}
		o += "\t"; o += std::to_string(top[0]); o += "\t"; o += std::to_string(top[1]); o += "\t"; o += std::to_string(top[1] - top[0]);
		for (int a = 0; a < 2; a++) { o += "\t"; o += (top[a] > 0 && rule[a] >= 0) ? std::to_string(rule[a]) : std::string("NA"); }
		o += "\t"; o += std::to_string(s.flags & 1); o += "\n";
	}
	return text_out(o, text, text_len);
}

// ---- variants on a sample's phased haplotypes (kernel: haplotype.hip) ------------------------------------------
// The planner: per record the consistent sets A_0 and A_1, per (focus, haplotype) a walk outwards from the focus through the applied
// neighbours until `flank` haplotype letters are collected on each side.  The window is never materialised for the device: it goes
// there as pieces (HapPiece) over the record and the uploaded ALT letters.  Every computed (entry, haplotype) is a unit of run_units,
// whether its walk met a neighbour or not: without one its sides are the plain windows' (plain_sides).
namespace {

// per haplotype and entry: 1 in A_h, 2 qualified but rejected for overlap, 3 qualifies but for its phase (an unphased heterozygote), else 0
struct HapSets { std::vector<uint8_t> status[2]; std::vector<int64_t> acc[2]; };

inline bool spans_meet(const fasim_variant& a, const fasim_variant& b) { return a.pos < b.pos + b.ref_len && b.pos < a.pos + a.ref_len; }

// the entries of record `rec` in the order (pos, line, index)
std::vector<int64_t> hap_order(const fasim_variant* vars, int64_t nvar, int32_t rec)
{
	std::vector<int64_t> ord;
	for (int64_t k = 0; k < nvar; k++) if (vars[k].rec == rec) ord.push_back(k);
	std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
		return vars[a].pos != vars[b].pos ? vars[a].pos < vars[b].pos : vars[a].line != vars[b].line ? vars[a].line < vars[b].line : a < b; });
	return ord;
}

// A_h of both haplotypes over one record's entries `ord`; status is indexed by entry (sized by the caller, zeros)
void hap_sets(const fasim_variant* vars, const fasim_genotype* gts, const uint8_t* matched, const std::vector<int64_t>& ord, HapSets& S)
{
	for (int h = 0; h < 2; h++) {
		int64_t end = INT64_MIN;      // of the last accepted span: the accepted spans are disjoint and sorted, so it is the largest
		for (int64_t k : ord) {
			const fasim_genotype& g = gts[k];
			if (g.hap[h] != 1) continue;
			if (vars[k].alt_len < 0 || (matched && !matched[k])) continue;
			if (!g.phased && !(g.hap[0] == 1 && g.hap[1] == 1)) { S.status[h][(size_t)k] = 3; continue; }
			if (vars[k].pos < end) { S.status[h][(size_t)k] = 2; continue; }
			S.status[h][(size_t)k] = 1; S.acc[h].push_back(k); end = vars[k].pos + vars[k].ref_len;
		}
	}
}

// the flanks of focus v on the haplotype whose consistent set is acc, in a record of len letters
void hap_walk(const fasim_variant* vars, const std::vector<int64_t>& acc, int64_t v, int64_t len, int32_t flank, HapSides& S)
{
	const fasim_variant& x = vars[v];
	auto skip = [&](int64_t u) { return vars[u].line == x.line || spans_meet(vars[u], x); };      // not an applied neighbour of v
	const int64_t first = std::lower_bound(acc.begin(), acc.end(), x.pos, [&](int64_t u, int64_t p) { return vars[u].pos < p; }) - acc.begin();
	int64_t need = flank, at = x.pos;
	bool cut = false;
	for (int64_t i = first - 1; need > 0; i--) {
		while (i >= 0 && skip(acc[(size_t)i])) i--;
		if (i < 0) { const int64_t take = std::min(need, at); if (take) S.left.push_back({ at - take, (int32_t)take, -1 }); at -= take; break; }
		const fasim_variant& y = vars[acc[(size_t)i]];
		const int64_t take = std::min(need, at - (y.pos + y.ref_len));
		if (take) { S.left.push_back({ at - take, (int32_t)take, -1 }); at -= take; need -= take; }
		if (!need) break;
		const int64_t t = std::min<int64_t>(need, y.alt_len);
		S.left.push_back({ y.alt_len - t, (int32_t)t, acc[(size_t)i] }); need -= t; S.applied++;
		if (t < y.alt_len) { cut = true; break; }
		at = y.pos;
	}
	S.edge_lo = cut || at > 0;
	std::reverse(S.left.begin(), S.left.end());
	need = flank; at = x.pos + x.ref_len; cut = false;
	for (size_t i = (size_t)first; need > 0; i++) {
		while (i < acc.size() && skip(acc[i])) i++;
		if (i >= acc.size()) { const int64_t take = std::min(need, len - at); if (take) S.right.push_back({ at, (int32_t)take, -1 }); at += take; break; }
		const fasim_variant& y = vars[acc[i]];
		const int64_t take = std::min(need, y.pos - at);
		if (take) { S.right.push_back({ at, (int32_t)take, -1 }); at += take; need -= take; }
		if (!need) break;
		const int64_t t = std::min<int64_t>(need, y.alt_len);
		S.right.push_back({ 0, (int32_t)t, acc[i] }); need -= t; S.applied++;
		if (t < y.alt_len) { cut = true; break; }
		at = y.pos + y.ref_len;
	}
	S.edge_hi = cut || at < len;
}

void pieces_letters(const fasim_variant* vars, const char* record, const std::vector<HPiece>& p, std::string& o)
{
	for (const HPiece& q : p) o.append(q.ent < 0 ? record + q.src : vars[q.ent].alt + q.src, (size_t)q.len);
}

inline bool pieces_equal(const std::vector<HPiece>& a, const std::vector<HPiece>& b)
{
	if (a.size() != b.size()) return false;
	for (size_t k = 0; k < a.size(); k++) if (a[k].src != b[k].src || a[k].len != b[k].len || a[k].ent != b[k].ent) return false;
	return true;
}

// do both haplotypes of a focus have the same windows?  The same pieces, or other pieces with the same letters and the same ends
bool hap_sides_equal(const fasim_variant* vars, const char* record, const HapSides* W, std::string (&w)[2])
{
	if (W[0].applied == 0 && W[1].applied == 0) return true;
	if (pieces_equal(W[0].left, W[1].left) && pieces_equal(W[0].right, W[1].right)) return true;
	if (W[0].edge_lo != W[1].edge_lo || W[0].edge_hi != W[1].edge_hi || pieces_len(W[0].left) != pieces_len(W[1].left) ||
		pieces_len(W[0].right) != pieces_len(W[1].right)) return false;
	for (int h = 0; h < 2; h++) { w[h].clear(); pieces_letters(vars, record, W[h].left, w[h]); pieces_letters(vars, record, W[h].right, w[h]); }
	return w[0] == w[1];
}

// carried, and flag bits 1 and 2, of focus v on haplotype h: one look at the record's entries within reach
void hap_context(const fasim_variant* vars, const fasim_genotype* gts, const std::vector<int64_t>& ord, const HapSets& S, int64_t v, int h,
	int32_t flank, int32_t& carried, int32_t& flags)
{
	const fasim_variant& x = vars[v];
	const int64_t reach = (int64_t)flank + FASIM_MAX_ALLELE;
	bool other_alt = false;
	auto it = std::lower_bound(ord.begin(), ord.end(), x.pos - reach, [&](int64_t u, int64_t p) { return vars[u].pos < p; });
	for (; it != ord.end() && vars[*it].pos <= x.pos + reach; ++it) {
		const int64_t u = *it;
		if (vars[u].line == x.line) { if (u != v && vars[u].pos == x.pos && gts[u].hap[h] == 1) other_alt = true; continue; }
		const uint8_t st = S.status[h][(size_t)u];
		if (st == 3) flags |= 2;
		if (st == 2 || (st == 1 && spans_meet(vars[u], x))) flags |= 4;
	}
	carried = gts[v].hap[h] == 1 ? 1 : gts[v].hap[h] < 0 ? -1 : other_alt ? 2 : 0;
}

}  // namespace

int fasim_haplotype_window(const fasim_variant* vars, const fasim_genotype* gts, int64_t nvar, const uint8_t* matched, int64_t rec_len,
	const char* record, int64_t v, int32_t hap, int32_t allele, int32_t flank, char** letters, int32_t* n, int32_t* v0, int32_t* edge)
{
	if (!vars || !gts || !record || !letters || !n || !v0 || !edge || v < 0 || v >= nvar || hap < 0 || hap > 1 || allele < 0 || allele > 1)
		return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (flank < 0 || flank > FASIM_MAX_FLANK) return fail(nullptr, FASIM_E_ARG, "flank %d lies outside [0, %d]", flank, FASIM_MAX_FLANK);
	const fasim_variant& x = vars[v];
	if (x.alt_len < 0) return fail(nullptr, FASIM_E_ARG, "variant %lld cannot be scored", (long long)v);
	for (int64_t k = 0; k < nvar; k++) {
		const fasim_variant& y = vars[k];
		if (y.rec != x.rec || y.alt_len < 0) continue;
		if (y.ref_len < 1 || y.ref_len > FASIM_MAX_ALLELE || y.alt_len < 1 || y.alt_len > FASIM_MAX_ALLELE || !y.alt || y.pos < 0 || y.pos > rec_len - y.ref_len)
			return fail(nullptr, FASIM_E_ARG, "variant %lld: alleles of 1 to %d letters inside the record of %lld nt", (long long)k, FASIM_MAX_ALLELE, (long long)rec_len);
	}
	try {
		const std::vector<int64_t> ord = hap_order(vars, nvar, x.rec);
		HapSets S;
		S.status[0].assign((size_t)nvar, 0); S.status[1].assign((size_t)nvar, 0);
		hap_sets(vars, gts, matched, ord, S);
		HapSides W;
		hap_walk(vars, S.acc[hap], v, rec_len, flank, W);
		std::string o;
		pieces_letters(vars, record, W.left, o);
		*v0 = (int32_t)o.size();
		if (allele) o.append(x.alt, (size_t)x.alt_len); else o.append(record + x.pos, (size_t)x.ref_len);
		pieces_letters(vars, record, W.right, o);
		*edge = (W.edge_lo ? 1 : 0) | (W.edge_hi ? 2 : 0);
		int64_t len = 0;
		const int rc = text_out(o, letters, &len);
		*n = (int32_t)len;
		return rc;
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
}

int fasim_haplotype_info(const fasim_variant* vars, const fasim_genotype* gts, int64_t nvar, const uint8_t* matched, int64_t rec_len,
	const char* record, int64_t v, int32_t flank, int32_t* carried, int32_t* applied, int32_t* flags)
{
	if (!vars || !gts || !record || !carried || !applied || !flags || v < 0 || v >= nvar) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	// (the checks of fasim_haplotype_window)
	char* letters = nullptr; int32_t n = 0, v0 = 0, edge = 0;
	const int rc = fasim_haplotype_window(vars, gts, nvar, matched, rec_len, record, v, 0, 0, flank, &letters, &n, &v0, &edge); if (rc) return rc;
	free(letters);
	try {
		const std::vector<int64_t> ord = hap_order(vars, nvar, vars[v].rec);
		HapSets S;
		S.status[0].assign((size_t)nvar, 0); S.status[1].assign((size_t)nvar, 0);
		hap_sets(vars, gts, matched, ord, S);
		HapSides W[2];
		std::string w[2];
		for (int h = 0; h < 2; h++) {
			flags[h] = 0;
			hap_context(vars, gts, ord, S, v, h, flank, carried[h], flags[h]);
			hap_walk(vars, S.acc[h], v, rec_len, flank, W[h]);
			applied[h] = W[h].applied;
		}
		if (hap_sides_equal(vars, record, W, w)) { flags[0] |= 8; flags[1] |= 8; }
		return FASIM_OK;
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
}

int fasim_score_haplotypes(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_variant* vars, const fasim_genotype* gts, const uint8_t* matched,
	int64_t nvar, int32_t flank, const fasim_params* pp, fasim_hap_score* out, fasim_variant_stats* stats)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nvar < 0 || (nvar > 0 && (!vars || !gts || !out))) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_variant_call(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, flank, pp, rs); if (rc) return rc;
	rc = check_variant_entries(E, vars, nvar, rec_len, nrec); if (rc) return rc;
	const char* host = rs.host(E);
	const double t0 = now_s();
	if (stats) memset(stats, 0, sizeof *stats);
	for (int64_t k = 0; k < (int64_t)nq * nvar; k++) {
		memset(&out[k], 0, sizeof out[k]);
		for (int h = 0; h < 2; h++) blank_score(out[k].hap[h]);
	}
	const std::vector<int> encs = enabled_encodings(*pp);
	struct Unit { int64_t v; int h; };
	try {
		// ---- the plan: the sides of every (entry, haplotype), and as units those that are computed ----
		std::vector<HapSides> sides((size_t)nvar * 2);
		std::vector<uint8_t> same((size_t)nvar, 0);      // both haplotypes have the windows of haplotype 0, which alone is computed
		std::vector<Unit> units;
		{
			std::vector<std::vector<int64_t>> by_rec((size_t)nrec);
			for (int64_t k = 0; k < nvar; k++) if (vars[k].rec >= 0 && vars[k].rec < nrec) by_rec[(size_t)vars[k].rec].push_back(k);
			HapSets S;
			S.status[0].assign((size_t)nvar, 0); S.status[1].assign((size_t)nvar, 0);
			std::string w[2];
			for (int32_t r = 0; r < nrec; r++) {
				std::vector<int64_t>& ord = by_rec[(size_t)r];
				if (ord.empty()) continue;
				std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
					return vars[a].pos != vars[b].pos ? vars[a].pos < vars[b].pos : vars[a].line != vars[b].line ? vars[a].line < vars[b].line : a < b; });
				S.acc[0].clear(); S.acc[1].clear();
				hap_sets(vars, gts, matched, ord, S);
				const char* record = host + rec_off[r];
				for (int64_t v : ord) {
					int32_t carried[2] = { 0, 0 }, flags[2] = { 0, 0 };
					for (int h = 0; h < 2; h++) hap_context(vars, gts, ord, S, v, h, flank, carried[h], flags[h]);
					for (int q = 0; q < nq; q++) for (int h = 0; h < 2; h++) { out[(size_t)q * (size_t)nvar + (size_t)v].carried[h] = carried[h]; out[(size_t)q * (size_t)nvar + (size_t)v].flags[h] = vars[v].alt_len < 0 ? 0 : flags[h]; }
					if (vars[v].alt_len < 0) continue;
					HapSides* W = &sides[(size_t)v * 2];
					for (int h = 0; h < 2; h++) hap_walk(vars, S.acc[h], v, rec_len[r], flank, W[h]);
					const bool eq = hap_sides_equal(vars, record, W, w);
					same[(size_t)v] = eq;
					for (int h = 0; h < (eq ? 1 : 2); h++) units.push_back({ v, h });
					for (int q = 0; q < nq; q++) for (int h = 0; h < 2; h++) out[(size_t)q * (size_t)nvar + (size_t)v].applied[h] = W[h].applied;
				}
			}
		}
		// ---- the units: k_hap_encode, then the kernels of section 19 ----
		UnitRun R{ E, "haplotypes", dna, rs.resident, rec_off, vars, &encs };
		const double ms0 = E->kernel_ms[4];
		const bool run = !units.empty() && !encs.empty();
		if (run) HIPOK(hipSetDevice(E->device));
		for (int q = 0; run && q < nq; q++) {
			rc = open_query(R, rnas[q], rna_lens[q]); if (rc) return rc;
			fasim_hap_score* row = out + (size_t)q * (size_t)nvar;
			rc = run_units(R, units.size(),
				[&](size_t k) { const Unit& U = units[k]; return ScoreUnit{ U.v, &sides[(size_t)U.v * 2 + (size_t)U.h], &row[U.v].hap[U.h] }; },
				[](size_t, int, const std::vector<TouchProb>&) { return FASIM_OK; });
			if (rc) return rc;
		}
		// ---- the computed haplotype into both, and the flags that the scores bring ----
		for (int q = 0; q < nq; q++) for (int64_t v = 0; v < nvar; v++) {
			if (vars[v].alt_len < 0 || vars[v].rec < 0 || vars[v].rec >= nrec) continue;
			fasim_hap_score& o = out[(size_t)q * (size_t)nvar + (size_t)v];
			if (same[(size_t)v]) o.hap[1] = o.hap[0];
			for (int h = 0; h < 2; h++) o.flags[h] |= (o.hap[h].flags & 1) | (same[(size_t)v] ? 8 : 0);
		}
		if (stats) { stats->problems = R.nprobs; stats->cells = R.cells; stats->kernel_s = run ? (E->kernel_ms[4] - ms0) * 1e-3 : 0.0; stats->total_s = now_s() - t0; }
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	return FASIM_OK;
}

int fasim_haplotypes_tsv(const fasim_variant* vars, const fasim_genotype* gts, const fasim_hap_score* scores, int64_t nvar, int32_t flank,
	const char* rna_name, const char* sample, const uint8_t* matched, char** text, int64_t* text_len)
{
	if (nvar < 0 || !rna_name || !sample || !text || !text_len || (nvar > 0 && (!vars || !gts || !scores))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "# fasim haplotypes lncRNA="; o += rna_name; o += " sample="; o += sample; o += " flank="; o += std::to_string(flank); o += "\n";
	o += "line\tchrom\tpos\tid\tref\talt\tgt";
	for (const char* h : { "h1", "h2" }) {
		const std::string pre = std::string("\t") + h + "_";
		o += pre + "carried" + pre + "applied";
		for (const char* c : CLASS_NAMES) { o += pre + c + "_ref" + pre + c + "_alt"; }
		for (const char* c : { "max_ref", "max_alt", "delta", "rule_ref", "rule_alt", "value", "flags" }) o += pre + c;
	}
	o += "\tdiplotype_max\n";
	const int ncol = 2 * (2 + 2 * FASIM_TRACK_CLASSES + 7) + 1;
	for (int64_t k = 0; k < nvar; k++) {
		const fasim_variant& x = vars[k];
		if (!x.chrom || !x.id || !x.ref || !x.alt) return fail(nullptr, FASIM_E_ARG, "variant %lld lacks a string", (long long)k);
		o += std::to_string(x.line); o += "\t"; o += x.chrom; o += "\t"; o += std::to_string(x.pos + 1); o += "\t"; o += x.id; o += "\t"; o += x.ref; o += "\t"; o += x.alt;
		const fasim_genotype& g = gts[k];
		o += "\t"; o += g.hap[0] < 0 ? "." : g.hap[0] ? "1" : "0"; o += g.phased ? "|" : "/"; o += g.hap[1] < 0 ? "." : g.hap[1] ? "1" : "0";
		if ((matched && !matched[k]) || x.alt_len < 0) { for (int c = 0; c < ncol; c++) o += "\tNA"; o += "\n"; continue; }
		const fasim_hap_score& S = scores[k];
		int value[2] = { -1, -1 };
		for (int h = 0; h < 2; h++) {
			const fasim_variant_score& s = S.hap[h];
			o += "\t"; o += std::to_string(S.carried[h]); o += "\t"; o += std::to_string(S.applied[h]);
			int top[2] = { 0, 0 }, rule[2] = { -1, -1 };
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
				o += "\t"; o += std::to_string(s.value[0][c]); o += "\t"; o += std::to_string(s.value[1][c]);
				for (int a = 0; a < 2; a++) if (s.value[a][c] > top[a]) { top[a] = s.value[a][c]; rule[a] = (s.enc[a][c] >= 0 && s.enc[a][c] < 48) ? enc_info(s.enc[a][c]).rule : -1; }
			}
			o += "\t"; o += std::to_string(top[0]); o += "\t"; o += std::to_string(top[1]); o += "\t"; o += std::to_string(top[1] - top[0]);
			for (int a = 0; a < 2; a++) { o += "\t"; o += (top[a] > 0 && rule[a] >= 0) ? std::to_string(rule[a]) : std::string("NA"); }
			if (S.carried[h] == 0 || S.carried[h] == 1) value[h] = top[S.carried[h]];
			o += "\t"; o += value[h] >= 0 ? std::to_string(value[h]) : std::string("NA");
			o += "\t"; o += std::to_string(S.flags[h]);
		}
		o += "\t"; o += (value[0] >= 0 && value[1] >= 0) ? std::to_string(std::max(value[0], value[1])) : std::string("NA"); o += "\n";
	}
	return text_out(o, text, text_len);
}
