// fasim-longtarget_amd/csrc/engine_variants.cpp -- fasim_score_variants: the triplex potential through variants (DESIGN.md section 19;
// kernels: variant.hip), and the table of `fasim --variants` (fasim_variants_tsv); fasim_score_variants_aligned: the same call with
// the alignment behind every score (section 21; kernel: variant_path.hip), its projection to the reference and its table.
//
// A variant is two allele windows, a window under an enabled encoding is a problem.  Per query the variants are cut into chunks by a
// fixed bound on buffer bytes; a chunk is: the windows' descriptions (and, for a streamed record, their letters) and the ALT letters
// up, k_var_encode, k_touch, k_touch_reduce, nine words per variant back.  Everything runs on the engine's own stream and in buffers
// of its own (vr_*): the engine's query, its scan buffers and its workers are not touched.
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
	if (nq < 1 || !rnas || !rna_lens || nvar < 0 || (nvar > 0 && (!vars || !out)) || !pp) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = record_set_open(E, dna, rec_off, rec_len, nrec, false, rs); if (rc) return rc;
	for (int32_t q = 0; q < nq; q++) {
		if (!rnas[q] || rna_lens[q] <= 0) return fail(E, FASIM_E_ARG, "empty query %d", q);
		if (rna_lens[q] > FASIM_MAX_QUERY) return fail(E, FASIM_E_UNSUPPORTED, "query %d has %d nt: the limit is %d", q, rna_lens[q], FASIM_MAX_QUERY);
	}
	if (pp->classicSim) return fail(E, FASIM_E_UNSUPPORTED, "variants are scored with the fastSIM scoring only: not with classicSim (-F)");
	if (flank < 0 || flank > FASIM_MAX_FLANK) return fail(E, FASIM_E_ARG, "flank %d lies outside [0, %d]", flank, FASIM_MAX_FLANK);
	rc = record_set_bounds(E, rs); if (rc) return rc;
	const bool resident = rs.resident;
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
	for (int64_t k = 0; k < (int64_t)nq * nvar; k++) {
		memset(&out[k], 0, sizeof out[k]);
		for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) out[k].enc[a][c] = -1;
	}
	const std::vector<int> encs = enabled_encodings(*pp);
	const int nenc = (int)encs.size();
	std::vector<int64_t> todo;                    // the variants that are scored
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
	int64_t nprobs = 0, cells = 0;
	try {
		for (int q = 0; q < nq; q++) {
			const int m = rna_lens[q];
			std::vector<uint8_t> qc((size_t)m);
			for (int i = 0; i < m; i++) qc[(size_t)i] = code2(rnas[q][i]);
			rc = upload(E, E->vr_q, qc.data(), qc.size()); if (rc) return rc;
			const bool rows_hbm = m > TOUCH_LDS_ROWS;
			const size_t row_bytes = (size_t)6 * (size_t)touch_state_rows(m);      // of one problem
			std::vector<HitOut> H;
			PathCtx PC;
			if (hits) {
				blank_hits(H);
				PC.E = E; PC.rna.assign(rnas[q], rnas[q] + m); PC.m = m; PC.encs = encs; PC.host = rs.host(E); PC.rec_off = rec_off; PC.rec_len = rec_len;
				PC.vars = vars; PC.flank = flank; PC.pc = *pp; PC.pc.ntMin = 1; PC.pc.ntMax = INT_MAX; PC.rows_hbm = rows_hbm; PC.row_bytes = row_bytes;
			}
			for (size_t w0 = 0; w0 < todo.size(); ) {
				std::vector<VarWindow> wins;
				std::vector<TouchProb> probs;
				std::vector<uint8_t> alts, letters;
				size_t tbytes = 0, w1 = w0;
				for (; w1 < todo.size(); w1++) {
					const fasim_variant& x = vars[todo[w1]];
					const int64_t len = rec_len[x.rec];
					const int64_t lo = std::max<int64_t>(0, x.pos - flank), hi = std::min<int64_t>(len, x.pos + x.ref_len + flank);
					const int pre = (int)(x.pos - lo), post = (int)(hi - x.pos - x.ref_len);
					const int n_al[2] = { pre + x.ref_len + post, pre + x.alt_len + post };
					const size_t need = (size_t)nenc * (size_t)(pad16(n_al[0]) + pad16(n_al[1]));
					if (w1 > w0 && (tbytes + need > VR_TCODE_BYTES || (int64_t)probs.size() + 2 * nenc > VR_MAX_PROBS ||
						(rows_hbm && (probs.size() + 2 * (size_t)nenc) * row_bytes > VR_ROW_BYTES))) break;
					// the record's letters of the window: in the resident buffer, or staged for this chunk
					int64_t src = rec_off[x.rec] + lo;
					if (!resident) { src = (int64_t)letters.size(); letters.insert(letters.end(), dna + rec_off[x.rec] + lo, dna + rec_off[x.rec] + hi); }
					const int edge_lo = lo > 0, edge_hi = hi < len;      // cut by the flank, not by the record's end
					for (int al = 0; al < 2; al++) {
						VarWindow W; W.src = src; W.pre = pre; W.ref_len = x.ref_len; W.post = post; W.alt_off = 0; W.alt_len = -1; W.pad = 0;
						if (al) { W.alt_off = (int32_t)alts.size(); W.alt_len = x.alt_len; alts.insert(alts.end(), x.alt, x.alt + x.alt_len); }
						const int n = n_al[al], v0 = pre, v1 = pre + (al ? x.alt_len : x.ref_len);
						for (int k = 0; k < nenc; k++) {
							const int enc = encs[(size_t)k];
							TouchProb P; P.tbase = (int64_t)tbytes; P.n = n; P.win = (int32_t)wins.size(); P.enc = enc;
							if (enc & 1) { P.v0 = n - v1; P.v1 = n - v0; P.edge = edge_hi | (edge_lo << 1); }
							else { P.v0 = v0; P.v1 = v1; P.edge = edge_lo | (edge_hi << 1); }
							probs.push_back(P);
							tbytes += (size_t)pad16(n);
							cells += (int64_t)m * n;
						}
						wins.push_back(W);
					}
				}
				const int np = (int)probs.size(), nv = (int)(w1 - w0);
				nprobs += np;
				if (alts.empty()) alts.push_back(0);
				if (E->vr_wins.ensure(wins.size() * sizeof(VarWindow)) != hipSuccess || E->vr_probs.ensure((size_t)np * sizeof(TouchProb)) != hipSuccess ||
					E->vr_alt.ensure(alts.size()) != hipSuccess || E->vr_tcodes.ensure(tbytes) != hipSuccess || E->vr_touch.ensure((size_t)np * sizeof(uint32_t)) != hipSuccess ||
					E->vr_out.ensure((size_t)nv * 9 * sizeof(uint32_t)) != hipSuccess || (!resident && E->vr_dna.ensure(letters.size() + 1) != hipSuccess) ||
					(rows_hbm && E->vr_rows.ensure((size_t)np * row_bytes) != hipSuccess)) {
					(void)hipGetLastError();
					return fail(E, FASIM_E_NOMEM, "variants: no device memory for a chunk of %d problems", np);
				}
				HIPOK(hipMemcpyAsync(E->vr_wins.p, wins.data(), wins.size() * sizeof(VarWindow), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_probs.p, probs.data(), (size_t)np * sizeof(TouchProb), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->vr_alt.p, alts.data(), alts.size(), hipMemcpyHostToDevice, E->st));
				if (!resident && !letters.empty()) HIPOK(hipMemcpyAsync(E->vr_dna.p, letters.data(), letters.size(), hipMemcpyHostToDevice, E->st));
				VarEncodeLaunch EL;
				EL.dna = resident ? E->dna_res.as<uint8_t>() : E->vr_dna.as<uint8_t>(); EL.alts = E->vr_alt.as<uint8_t>(); EL.wins = E->vr_wins.as<VarWindow>();
				EL.probs = E->vr_probs.as<TouchProb>(); EL.nprob = np; EL.enc_lut = E->enc_lut.as<uint8_t>(); EL.tcodes = E->vr_tcodes.as<uint8_t>();
				hipError_t he = launch_var_encode(EL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "variants (encode) launch failed: %s", hipGetErrorString(he));
				TouchLaunch TL;
				TL.tcodes = E->vr_tcodes.as<uint8_t>(); TL.qcodes = E->vr_q.as<uint8_t>(); TL.m = m; TL.probs = E->vr_probs.as<TouchProb>(); TL.nprob = np;
				TL.rows = rows_hbm ? E->vr_rows.as<uint16_t>() : nullptr; TL.out = E->vr_touch.as<uint32_t>();
				{ TimedScope ts(E, 4); he = launch_touch(TL, E->st); }
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "variants (touch) launch failed: %s", hipGetErrorString(he));
				TouchReduceLaunch RL;
				RL.touch = E->vr_touch.as<uint32_t>(); RL.nvar = nv; RL.nenc = nenc; RL.out = E->vr_out.as<uint32_t>();
				memset(RL.enc, 0, sizeof RL.enc);
				for (int k = 0; k < nenc; k++) RL.enc[k] = (uint8_t)encs[(size_t)k];
				he = launch_touch_reduce(RL, E->st);
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "variants (reduce) launch failed: %s", hipGetErrorString(he));
				std::vector<uint32_t> words((size_t)nv * 9);
				HIPOK(hipMemcpyAsync(words.data(), E->vr_out.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
				HIPOK(hipStreamSynchronize(E->st));
				drain_timed(E);
				for (int k = 0; k < nv; k++) {
					fasim_variant_score& s = out[(size_t)q * (size_t)nvar + (size_t)todo[w0 + (size_t)k]];
					for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
						const uint32_t w = words[(size_t)k * 9 + (size_t)a * 4 + (size_t)c];
						s.value[a][c] = (int32_t)(w >> 9);
						s.enc[a][c] = (w >> 9) ? (int32_t)(w & 0xff) : -1;
					}
					s.flags = (int32_t)(words[(size_t)k * 9 + 8] & 1);
				}
				if (hits) { rc = trace_chunk(PC, probs, todo.data() + w0, nv, out + (size_t)q * (size_t)nvar, H); if (rc) return rc; }
				w0 = w1;
			}
			if (hits && !(hits[q] = pack_hits(H))) return fail(E, FASIM_E_NOMEM, "out of memory");
		}
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (stats) { stats->problems = nprobs; stats->cells = cells; stats->kernel_s = (E->kernel_ms[4] - ms0) * 1e-3; stats->total_s = now_s() - t0; }
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
