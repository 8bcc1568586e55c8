// fasim-longtarget_amd/csrc/engine_variants.cpp -- fasim_score_variants: the triplex potential through variants (DESIGN.md section 19;
// kernels: variant.hip), and the table of `fasim --variants` (fasim_variants_tsv).
//
// A variant is two allele windows, a window under an enabled encoding is a problem.  Per query the variants are cut into chunks by a
// fixed bound on buffer bytes; a chunk is: the windows' descriptions (and, for a streamed record, their letters) and the ALT letters
// up, k_var_encode, k_touch, k_touch_reduce, nine words per variant back.  Everything runs on the engine's own stream and in buffers
// of its own (vr_*): the engine's query, its scan buffers and its workers are not touched.
#include "engine.h"

namespace {

constexpr size_t VR_TCODE_BYTES = (size_t)16 << 20;      // target codes of a chunk
constexpr size_t VR_ROW_BYTES = (size_t)256 << 20;       // HBM row state of a chunk (queries above TOUCH_LDS_ROWS)
constexpr int64_t VR_MAX_PROBS = 1 << 20;                // problems of a chunk

inline int pad16(int n) { return (n + 15) & ~15; }

}  // namespace

int fasim_score_variants(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_variant* vars, int64_t nvar, int32_t flank,
	const fasim_params* pp, fasim_variant_score* out, fasim_variant_stats* stats)
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
	for (int64_t k = 0; k < (int64_t)nq * nvar; k++) {
		memset(&out[k], 0, sizeof out[k]);
		for (int a = 0; a < 2; a++) for (int c = 0; c < FASIM_TRACK_CLASSES; c++) out[k].enc[a][c] = -1;
	}
	const std::vector<int> encs = enabled_encodings(*pp);
	const int nenc = (int)encs.size();
	std::vector<int64_t> todo;                    // the variants that are scored
	for (int64_t v = 0; v < nvar; v++) if (vars[v].alt_len >= 0) todo.push_back(v);
	if (todo.empty() || nenc == 0) { if (stats) stats->total_s = now_s() - t0; return FASIM_OK; }
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
				w0 = w1;
			}
		}
	} catch (const std::bad_alloc&) { (void)hipStreamSynchronize(E->st); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (stats) { stats->problems = nprobs; stats->cells = cells; stats->kernel_s = (E->kernel_ms[4] - ms0) * 1e-3; stats->total_s = now_s() - t0; }
	return FASIM_OK;
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
