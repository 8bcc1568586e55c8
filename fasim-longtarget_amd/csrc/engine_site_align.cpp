// fasim-longtarget_amd/csrc/engine_site_align.cpp -- fasim_scan_records_sites_aligned: the second phase of a sites call, which gives
// every site its hit (kernels: site_align.hip), and the host functions on hit lists (merge, table, free).
//
// The sites of a call are final only after the host sweep that joins the kernel's runs over slices, segments and max_gap, so the
// hits are a phase of their own behind fasim_scan_records_sites: per query the sites of all records become a list of problems
// (unit, column of the peak, value) -- one per selected segment that covers the peak, so that the smallest segment that holds the
// value can be chosen afterwards --, the list is cut into chunks, and a chunk is: encode its units on the host and upload them,
// k_site_ends, the end and start cells back, k_site_path for the rectangles, the CIGARs back, convert_triplex on the host.
// The hits of oligo sites (fasim_scan_oligos_aligned, section 18) are the same phase with k_site_ends_short in k_site_ends' place.
#include <climits>
#include <unordered_map>

#include "engine.h"

namespace {

struct Work { int32_t site, unit, n, jp, value, enc, level; int64_t seg, soff, key; };      // one problem: site index in the query's flat list; level = its rank among the site's covering segments; key = the unit

} // namespace

void hit_clear(HitOut& H, int enc)
{
	H.t = HostTriplex(); H.t.stari = H.t.endi = H.t.starj = H.t.endj = H.t.strand = H.t.reverse = H.t.rule = H.t.nt = 0;
	H.t.score = H.t.identity = H.t.tri_score = 0.0f; H.t.seg = -1; H.t.enc = enc;
}

void path_hit(HitOut& H, const uint32_t* cig, int len, int value, const std::string& rna, const char* seg, int n, int enc, long origin, const fasim_params& pc, int seg_id)
{
	H.cigar.assign(cig, cig + len);
	std::reverse(H.cigar.begin(), H.cigar.end());      // the traceback wrote the last operation first
	AlignResult al;
	al.sw_score = value; al.ref_begin = H.j0; al.ref_end = H.j1; al.query_begin = H.i0; al.query_end = H.i1; al.cigar_len = len;
	std::vector<HostTriplex> one;
	convert_triplex(al, H.cigar.data(), rna, seg, n, enc, origin, pc, one, only_acgtn(seg, n), true);
	if (one.empty()) { H.cigar.clear(); return; }
	H.t = std::move(one[0]); H.t.seg = seg_id; H.t.enc = enc; H.aligned = true;
}

// the hit list of one (query, record) from its hits in site order
fasim_site_hits* pack_hits(const std::vector<HitOut>& v)
{
	fasim_site_hits* h = (fasim_site_hits*)calloc(1, sizeof(fasim_site_hits));
	if (!h) return nullptr;
	const size_t n = v.size();
	size_t pool = 1, ncig = 0;
	for (const HitOut& x : v) { if (x.aligned) { pool += x.t.tfo.size() + x.t.tts.size() + 2; ncig += x.cigar.size(); } }
	h->n = (int64_t)n;
	h->t = (fasim_triplex*)calloc(std::max<size_t>(1, n), sizeof(fasim_triplex));
	h->q_begin = (int32_t*)calloc(std::max<size_t>(1, n), sizeof(int32_t)); h->q_end = (int32_t*)calloc(std::max<size_t>(1, n), sizeof(int32_t));
	h->t_begin = (int32_t*)calloc(std::max<size_t>(1, n), sizeof(int32_t)); h->t_end = (int32_t*)calloc(std::max<size_t>(1, n), sizeof(int32_t));
	h->cigar_off = (int64_t*)calloc(std::max<size_t>(1, n), sizeof(int64_t)); h->cigar_len = (int32_t*)calloc(std::max<size_t>(1, n), sizeof(int32_t));
	h->cigar = (uint32_t*)calloc(std::max<size_t>(1, ncig), sizeof(uint32_t));
	h->pool = (char*)calloc(pool, 1);
	if (!h->t || !h->q_begin || !h->q_end || !h->t_begin || !h->t_end || !h->cigar_off || !h->cigar_len || !h->cigar || !h->pool) { site_hits_free(h); return nullptr; }
	h->pool_len = (int64_t)pool;
	size_t off = 1, coff = 0;                     // pool[0] = the empty string of the unaligned hits
	for (size_t i = 0; i < n; i++) {
		const HitOut& x = v[i];
		fasim_triplex& r = h->t[i];
		const HostTriplex& t = x.t;
		r.stari = t.stari; r.endi = t.endi; r.starj = t.starj; r.endj = t.endj; r.strand = t.strand; r.reverse = t.reverse;
		r.rule = t.rule; r.nt = t.nt; r.score = t.score; r.identity = t.identity; r.tri_score = t.tri_score; r.seg = t.seg; r.enc = t.enc;
		h->q_begin[i] = x.i0; h->q_end[i] = x.i1; h->t_begin[i] = x.j0; h->t_end[i] = x.j1;
		h->cigar_off[i] = (int64_t)coff;
		if (x.empty) continue;                        // (cigar_len 0, the empty string)
		if (!x.aligned) { h->cigar_len[i] = -1; h->unaligned++; continue; }
		h->cigar_len[i] = (int32_t)x.cigar.size();
		memcpy(h->cigar + coff, x.cigar.data(), x.cigar.size() * sizeof(uint32_t)); coff += x.cigar.size();
		r.tfo_off = (int64_t)off; memcpy(h->pool + off, t.tfo.c_str(), t.tfo.size() + 1); off += t.tfo.size() + 1;
		r.tts_off = (int64_t)off; memcpy(h->pool + off, t.tts.c_str(), t.tts.size() + 1); off += t.tts.size() + 1;
	}
	return h;
}

void site_hits_free(fasim_site_hits* h)
{
	if (!h) return;
	free(h->t); free(h->q_begin); free(h->q_end); free(h->t_begin); free(h->t_end); free(h->cigar_off); free(h->cigar_len); free(h->cigar); free(h->pool);
	free(h);
}

int run_site_align(fasim_engine* E, SiteAlignReq& R)
{
	HIPOK(hipSetDevice(E->device));
	const fasim_params& p = R.p;
	const int nrec = R.nrec, nquery = (int)R.queries.size();
	const int64_t step = p.cutLength - p.overlapLength;
	const int tstride = (p.cutLength + 15) & ~15;
	const SegRange range = segment_range(R.rec_len, nrec, R.seg_first, R.seg_count, p);
	const std::vector<int64_t>& rec_first = range.rec_first;
	const int64_t seg_first = range.seg_first, seg_count = range.seg_count;
	static const std::vector<uint8_t> lut = [] { std::vector<uint8_t> v(48 * 256); build_enc_lut(v.data()); return v; }();
	fasim_params pc = p; pc.ntMin = 1; pc.ntMax = INT_MAX;      // hits are never filtered by length
	const bool prof = [] { const char* e = getenv("FASIM_PROFILE"); return e && atoi(e) != 0; }();
	const double ms0 = E->kernel_ms[4];
	int64_t nsites = 0, nprobs = 0, cells = 0;
	try {
		for (int q = 0; q < nquery; q++) {
			const std::string& rna = R.queries[(size_t)q];
			const int m = (int)rna.size(), npad = 16 * ((m + 15) / 16) - m;
			std::vector<uint8_t> qc((size_t)m);
			for (int i = 0; i < m; i++) qc[(size_t)i] = code2(rna[(size_t)i]);
			int rc = upload(E, E->sa_q, qc.data(), qc.size()); if (rc) return rc;
			// the query's sites, flat: (record, index) in record order; one HitOut each
			std::vector<std::vector<HitOut>> hits((size_t)nrec);
			std::vector<std::pair<int, int>> flat;
			std::vector<Work> all;
			int max_level = 0;
			for (int r = 0; r < nrec; r++) {
				const fasim_sites* S = R.sites[(size_t)q * nrec + r];
				hits[(size_t)r].resize((size_t)S->n);
				const int64_t nseg = rec_first[(size_t)r + 1] - rec_first[(size_t)r];
				for (int64_t k = 0; k < S->n; k++) {
					const fasim_site& x = S->s[k];
					HitOut& H = hits[(size_t)r][(size_t)k];
					hit_clear(H, x.enc);
					const int site = (int)flat.size();
					flat.emplace_back(r, (int)k);
					if (x.value >= 16383 || x.value < 1 || x.enc < 0 || x.enc >= 48) continue;      // a saturated unit: no hit
					if (p.cutLength > SITE_ALIGN_MAX_COLS) continue;      // the kernels' 16-bit state holds units of that many columns
					// the selected segments that cover pos, by ascending index
					int64_t s0 = x.pos < p.cutLength ? 0 : (x.pos - p.cutLength) / step + 1;
					int level = 0;
					for (int64_t s = s0; s < nseg && s * step <= x.pos; s++) {
						const int64_t g = rec_first[(size_t)r] + s, a = s * step;
						const int n = (int)std::min<int64_t>(p.cutLength, R.rec_len[r] - a);
						if (x.pos >= a + n || g < seg_first || g >= seg_first + seg_count) continue;
						const int64_t soff = R.rec_off[r] + a;
						if (same_seq(R.dna + soff, n)) continue;
						Work w; w.site = site; w.unit = -1; w.n = n; w.enc = x.enc; w.seg = s; w.soff = soff; w.value = x.value;
						w.jp = (x.enc & 1) ? n - 1 - (int)(x.pos - a) : (int)(x.pos - a);
						w.level = level++; w.key = g * 48 + x.enc;
						max_level = std::max(max_level, w.level);
						all.push_back(w);
					}
				}
			}
			nsites += (int64_t)flat.size(); 
			// chunks of problems: at most 4 096 problems (short_query: 262 144, a problem is a lane there), 256 MB of units, 512 MB of row state
			const size_t max_units = std::max<size_t>(1, ((size_t)256 << 20) / (size_t)tstride);
			const bool rows_hbm = m > SITE_ALIGN_LDS_ROWS;
			size_t max_probs = R.short_query ? (size_t)262144 : rows_hbm ? std::max<size_t>(1, std::min<size_t>(4096, ((size_t)512 << 20) / ((size_t)6 * m))) : 4096;
			if (E->opt_site_chunk > 0) max_probs = std::min<size_t>(max_probs, (size_t)E->opt_site_chunk);      // (option site_chunk: tests of the chunk loop)
			const int64_t short_cells = R.short_query ? (int64_t)(m + npad) * (site_short_warm(m) + 16) : 0;      // pass (i) of k_site_ends_short: the same for every problem
			std::vector<char> done(flat.size(), 0);      // the site has its unit: later (larger) segments are not looked at
			// level by level: the second covering segment of a site is a problem only where the first does not hold the value;
			// within a level by (unit, column), so that the problems of a unit share its upload
			for (int level = 0; level <= max_level; level++) {
			std::vector<Work> work;
			for (const Work& w : all) if (w.level == level && !done[(size_t)w.site]) work.push_back(w);
			std::sort(work.begin(), work.end(), [](const Work& a, const Work& b) { return a.key != b.key ? a.key < b.key : (a.jp != b.jp ? a.jp < b.jp : a.site < b.site); });
			nprobs += (int64_t)work.size();
			for (size_t w0 = 0; w0 < work.size(); ) {
				std::unordered_map<int64_t, int> slot;
				std::vector<uint8_t> tcodes;
				std::vector<SiteAlignProb> probs;
				size_t w1 = w0;
				for (; w1 < work.size() && probs.size() < max_probs; w1++) {
					Work& w = work[w1];
					const int64_t key = w.key;
					auto it = slot.find(key);
					if (it == slot.end()) {
						if (slot.size() >= max_units) break;
						const int u = (int)slot.size();
						it = slot.emplace(key, u).first;
						tcodes.resize((size_t)(u + 1) * tstride, 4);
						const uint8_t* l = lut.data() + (size_t)w.enc * 256;
						const char* seg = R.dna + w.soff;
						uint8_t* dst = tcodes.data() + (size_t)u * tstride;
						if (w.enc & 1) for (int c = 0; c < w.n; c++) dst[c] = l[(uint8_t)seg[w.n - 1 - c]];
						else for (int c = 0; c < w.n; c++) dst[c] = l[(uint8_t)seg[c]];
					}
					w.unit = it->second;
					SiteAlignProb P; P.tbase = (int64_t)w.unit * tstride; P.n = w.n; P.jp = w.jp; P.value = w.value; P.pad = 0;
					probs.push_back(P);
					cells += R.short_query ? short_cells : (int64_t)m * (w.jp + 1);
				}
				const int np = (int)probs.size();
				if (E->sa_tcodes.ensure(tcodes.size()) != hipSuccess || E->sa_probs.ensure((size_t)np * sizeof(SiteAlignProb)) != hipSuccess ||
					E->sa_ends.ensure((size_t)np * sizeof(SiteAlignEnds)) != hipSuccess || (rows_hbm && E->sa_rows.ensure((size_t)np * 6 * (size_t)m) != hipSuccess)) {
					(void)hipGetLastError();
					return fail(E, FASIM_E_NOMEM, "site hits: no device memory for a chunk of %d problems", np);
				}
				HIPOK(hipMemcpyAsync(E->sa_tcodes.p, tcodes.data(), tcodes.size(), hipMemcpyHostToDevice, E->st));
				HIPOK(hipMemcpyAsync(E->sa_probs.p, probs.data(), (size_t)np * sizeof(SiteAlignProb), hipMemcpyHostToDevice, E->st));
				SiteEndsLaunch L;
				L.tcodes = E->sa_tcodes.as<uint8_t>(); L.qcodes = E->sa_q.as<uint8_t>(); L.m = m; L.npad = npad;
				L.probs = E->sa_probs.as<SiteAlignProb>(); L.nprob = np; L.rows = rows_hbm ? E->sa_rows.as<int16_t>() : nullptr;
				L.ends = E->sa_ends.as<SiteAlignEnds>();
				hipError_t he;
				{ TimedScope ts(E, 4); he = R.short_query ? launch_site_ends_short(L, E->st) : launch_site_ends(L, E->st); }
				if (he != hipSuccess) return fail(E, FASIM_E_HIP, "site hits (ends) launch failed: %s", hipGetErrorString(he));
				std::vector<SiteAlignEnds> ends((size_t)np);
				HIPOK(hipMemcpyAsync(ends.data(), E->sa_ends.p, (size_t)np * sizeof(SiteAlignEnds), hipMemcpyDeviceToHost, E->st));
				HIPOK(hipStreamSynchronize(E->st));
				drain_timed(E);
				// per site the first problem (smallest segment) whose unit holds the value; its rectangle becomes a path item
				std::vector<SitePathItem> items;
				std::vector<size_t> item_work;
				for (int k = 0; k < np; k++) {
					const Work& w = work[w0 + (size_t)k];
					const SiteAlignEnds& e = ends[(size_t)k];
					if (done[(size_t)w.site] || e.i1 < 0) continue;
					done[(size_t)w.site] = 1;
					HitOut& H = hits[(size_t)flat[(size_t)w.site].first][(size_t)flat[(size_t)w.site].second];
					H.t.seg = (int)w.seg; H.i1 = e.i1; H.j1 = e.j1; H.i0 = e.i0; H.j0 = e.j0;
					if (e.i0 < 0 || e.j0 < 0 || e.i0 > e.i1 || e.j0 > e.j1 || e.i1 >= m || e.j1 >= w.n) continue;
					const int64_t rows = e.i1 - e.i0 + 1, cols = e.j1 - e.j0 + 1;
					cells += (int64_t)(e.i1 + 1) * cols;
					if (rows > SITE_ALIGN_LDS_ROWS || rows * cols > SITE_ALIGN_MAX_CELLS) continue;      // left unaligned
					SitePathItem I; I.dir_off = 0; I.prob = k; I.i0 = e.i0; I.i1 = e.i1; I.j0 = e.j0; I.j1 = e.j1; I.cig_off = 0; I.cig_cap = (int32_t)(rows + cols); I.pad = 0;
					items.push_back(I); item_work.push_back(w0 + (size_t)k);
				}
				// path launches: at most 512 MB of direction bytes each
				for (size_t a = 0; a < items.size(); ) {
					const LaunchCut cut = cut_launch(items, a, (int64_t)512 << 20, (int64_t)1 << 28, [](const SitePathItem& I) { return std::pair<int64_t, int64_t>(I.i1 - I.i0 + 1, I.j1 - I.j0 + 1); });
					cells += cut.dir_total;
					const int ni = (int)(cut.end - a);
					if (E->sa_items.ensure((size_t)ni * sizeof(SitePathItem)) != hipSuccess || E->sa_dirs.ensure((size_t)cut.dir_total) != hipSuccess ||
						E->sa_cigar.ensure((size_t)cut.cig_total * sizeof(uint32_t)) != hipSuccess || E->sa_ciglen.ensure((size_t)ni * sizeof(int32_t)) != hipSuccess) {
						(void)hipGetLastError();
						return fail(E, FASIM_E_NOMEM, "site hits: no device memory for the direction bytes of %d paths (%lld bytes)", ni, (long long)cut.dir_total);
					}
					HIPOK(hipMemcpyAsync(E->sa_items.p, items.data() + a, (size_t)ni * sizeof(SitePathItem), hipMemcpyHostToDevice, E->st));
					SitePathLaunch PL;
					PL.tcodes = E->sa_tcodes.as<uint8_t>(); PL.qcodes = E->sa_q.as<uint8_t>(); PL.probs = E->sa_probs.as<SiteAlignProb>();
					PL.items = E->sa_items.as<SitePathItem>(); PL.nitem = ni; PL.max_rows = cut.max_rows;
					PL.dirs = E->sa_dirs.as<uint8_t>(); PL.cigar = E->sa_cigar.as<uint32_t>(); PL.cigar_len = E->sa_ciglen.as<int32_t>();
					{ TimedScope ts(E, 4); he = launch_site_path(PL, E->st); }
					if (he != hipSuccess) return fail(E, FASIM_E_HIP, "site hits (path) launch failed: %s", hipGetErrorString(he));
					std::vector<int32_t> clen((size_t)ni);
					std::vector<uint32_t> cig((size_t)cut.cig_total);
					HIPOK(hipMemcpyAsync(clen.data(), E->sa_ciglen.p, (size_t)ni * sizeof(int32_t), hipMemcpyDeviceToHost, E->st));
					HIPOK(hipMemcpyAsync(cig.data(), E->sa_cigar.p, (size_t)cut.cig_total * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
					HIPOK(hipStreamSynchronize(E->st));
					drain_timed(E);
					for (int k = 0; k < ni; k++) {
						const SitePathItem& I = items[a + (size_t)k];
						const Work& w = work[item_work[a + (size_t)k]];
						if (clen[(size_t)k] < 1 || clen[(size_t)k] > I.cig_cap) continue;
						HitOut& H = hits[(size_t)flat[(size_t)w.site].first][(size_t)flat[(size_t)w.site].second];
						path_hit(H, cig.data() + I.cig_off, clen[(size_t)k], w.value, rna, R.dna + w.soff, w.n, w.enc, (long)(w.seg * step), pc, (int)w.seg);
					}
					a = cut.end;
				}
				w0 = w1;
			}
			}
			for (int r = 0; r < nrec; r++) {
				fasim_site_hits* h = pack_hits(hits[(size_t)r]);
				if (!h) return fail(E, FASIM_E_NOMEM, "out of memory");
				R.hits[(size_t)q * nrec + r] = h;
			}
		}
	} catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (prof) fprintf(stderr, "[fasim prof] site hits: %lld sites, %lld problems, %lld cells, %.3f ms of kernels\n", (long long)nsites, (long long)nprobs,
		(long long)cells, E->kernel_ms[4] - ms0);
	return FASIM_OK;
}

void fasim_site_hits_free(fasim_site_hits* h) { site_hits_free(h); }

int fasim_scan_records_sites_aligned(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_result** out_results, fasim_sites** out_sites, fasim_site_hits** out_hits, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_hits) return fail(E, FASIM_E_ARG, "bad arguments");
	// first phase: the sites call itself, refusals included (its results, sites and totals are this call's)
	RecordSet rs;
	int rc = scan_records_sites(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_results, out_sites, totals, rs);
	if (rc) return rc;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec;
	for (size_t o = 0; o < nout; o++) out_hits[o] = nullptr;
	SiteAlignReq R;
	R.dna = rs.host(E); R.rec_off = rs.rec_off; R.rec_len = rs.rec_len; R.nrec = nrec; R.seg_first = seg_first; R.seg_count = seg_count;
	R.p = *pp; R.sites = out_sites; R.hits = out_hits;
	try {
		if (nq == 0) R.queries.push_back(E->rna);
		else for (int q = 0; q < nq; q++) R.queries.emplace_back(rnas[q], rnas[q] + rna_lens[q]);
		rc = run_site_align(E, R);
	} catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (rc) {
		(void)hipStreamSynchronize(E->st);
		for (size_t o = 0; o < nout; o++) {
			site_hits_free(out_hits[o]); out_hits[o] = nullptr;
			fasim_sites_free(out_sites[o]); out_sites[o] = nullptr;
			if (out_results) { fasim_result_free(out_results[o]); out_results[o] = nullptr; }
		}
	}
	return rc;
}

int fasim_site_hits_merge(const fasim_sites* const* sites, const fasim_site_hits* const* hits, int32_t nparts, fasim_sites** out_sites, fasim_site_hits** out_hits)
{
	if (!sites || !hits || nparts < 1 || !out_hits) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out_hits = nullptr;
	if (out_sites) *out_sites = nullptr;
	for (int k = 0; k < nparts; k++) {
		if (!sites[k] || !hits[k] || hits[k]->n < 0) return fail(nullptr, FASIM_E_ARG, "bad part %d", k);
		if (hits[k]->n != sites[k]->n) return fail(nullptr, FASIM_E_ARG, "part %d has %lld sites and %lld hits", k, (long long)sites[k]->n, (long long)hits[k]->n);
	}
	fasim_sites* M = nullptr;
	const int rc = fasim_sites_merge(sites, nparts, &M);
	if (rc) return rc;
	fasim_site_hits* h = nullptr;
	try {
		// the parts' sites by (class, start): every one lies inside exactly one merged site
		struct Ref { int32_t cls; int64_t start; int part; int64_t idx; };
		std::vector<Ref> refs;
		for (int k = 0; k < nparts; k++) for (int64_t i = 0; i < sites[k]->n; i++) refs.push_back({ sites[k]->s[i].cls, sites[k]->s[i].start, k, i });
		std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return a.cls != b.cls ? a.cls < b.cls : (a.start != b.start ? a.start < b.start : (a.part != b.part ? a.part < b.part : a.idx < b.idx)); });
		std::vector<HitOut> v((size_t)M->n);
		for (int64_t i = 0; i < M->n; i++) {
			const fasim_site& x = M->s[i];
			HitOut& H = v[(size_t)i];
			hit_clear(H, x.enc);
			auto it = std::lower_bound(refs.begin(), refs.end(), x, [](const Ref& a, const fasim_site& s) { return a.cls != s.cls ? a.cls < s.cls : a.start < s.start; });
			int bp = -1; int64_t bi = -1;
			for (; it != refs.end() && it->cls == x.cls && it->start < x.end; ++it) {
				const fasim_site& y = sites[it->part]->s[it->idx];
				if (y.value != x.value || y.pos != x.pos || y.enc != x.enc) continue;
				const fasim_site_hits* hp = hits[it->part];
				if (bp < 0) { bp = it->part; bi = it->idx; continue; }
				const fasim_site_hits* hb = hits[bp];
				const bool a_new = hp->cigar_len[it->idx] >= 0, a_old = hb->cigar_len[bi] >= 0;
				const int s_new = hp->t[it->idx].seg, s_old = hb->t[bi].seg;
				if ((a_new && !a_old) || (a_new == a_old && s_new >= 0 && (s_old < 0 || s_new < s_old))) { bp = it->part; bi = it->idx; }
			}
			if (bp < 0) continue;
			const fasim_site_hits* hb = hits[bp];
			const fasim_triplex& r = hb->t[bi];
			H.t.stari = r.stari; H.t.endi = r.endi; H.t.starj = r.starj; H.t.endj = r.endj; H.t.strand = r.strand; H.t.reverse = r.reverse;
			H.t.rule = r.rule; H.t.nt = r.nt; H.t.score = r.score; H.t.identity = r.identity; H.t.tri_score = r.tri_score; H.t.seg = r.seg; H.t.enc = r.enc;
			H.i0 = hb->q_begin[bi]; H.i1 = hb->q_end[bi]; H.j0 = hb->t_begin[bi]; H.j1 = hb->t_end[bi];
			if (hb->cigar_len[bi] >= 0) {
				H.aligned = true;
				H.cigar.assign(hb->cigar + hb->cigar_off[bi], hb->cigar + hb->cigar_off[bi] + hb->cigar_len[bi]);
				H.t.tfo = hb->pool + r.tfo_off; H.t.tts = hb->pool + r.tts_off;
			}
		}
		h = pack_hits(v);
	} catch (const std::bad_alloc&) { h = nullptr; }
	if (!h) { fasim_sites_free(M); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	*out_hits = h;
	if (out_sites) *out_sites = M; else fasim_sites_free(M);
	return FASIM_OK;
}

int fasim_site_hits_tsv(const fasim_sites* s, const fasim_site_hits* h, const char* chr, int64_t start_genome, const char* rna_name,
	const char* record_name, int32_t header, char** text, int64_t* text_len)
{
	if (!s || !h || !chr || !rna_name || !text || !text_len || s->n < 0 || (s->n > 0 && !s->s) || h->n != s->n) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	const int64_t sg = start_genome - 1;                  // 0-based genome position of the record's first base
	std::string o;
	char b[96];
	if (header) {
		o += "# fasim site hits lncRNA="; o += rna_name; o += " min_value="; o += std::to_string(s->min_value); o += " max_gap="; o += std::to_string(s->max_gap); o += "\n";
		o += "chrom\ttts_start\ttts_end\tclass\tvalue\tstrand\trule\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tTFO\tTTS";
		if (record_name) o += "\tname";
		o += "\n";
	}
	for (int64_t i = 0; i < s->n; i++) {
		const fasim_site& x = s->s[i];
		const fasim_triplex& t = h->t[i];
		if (x.cls < 0 || x.cls >= FASIM_TRACK_CLASSES) return fail(nullptr, FASIM_E_ARG, "site %lld has class %d", (long long)i, x.cls);
		const bool al = h->cigar_len[i] >= 0;
		// DNA bases of the hit, 0-based half-open: the mirrored encodings carry starj 0-based (fastsim.h:389-396), the others 1-based
		int64_t a = x.start, e = x.end;
		if (al) { if (t.enc & 1) { a = t.starj; e = (int64_t)t.endj + 1; } else { a = (int64_t)t.starj - 1; e = t.endj; } }
		o += chr;
		int n = snprintf(b, sizeof b, "\t%lld\t%lld\t%s\t%d\t%c", (long long)(sg + a), (long long)(sg + e), CLASS_NAMES[x.cls], x.value, (x.cls == 0 || x.cls == 3) ? '+' : '-');
		o.append(b, (size_t)n);
		if (!al) o += "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA";
		else {
			n = snprintf(b, sizeof b, "\t%d\t%d\t%d\t%d\t%g\t%g\t", t.rule, t.stari, t.endi, t.nt, (double)t.identity, (double)t.tri_score);
			o.append(b, (size_t)n);
			for (int32_t k = 0; k < h->cigar_len[i]; k++) {
				const uint32_t c = h->cigar[h->cigar_off[i] + k];
				n = snprintf(b, sizeof b, "%u%c", c >> 4, "MID"[(c & 15) < 3 ? (c & 15) : 0]);
				o.append(b, (size_t)n);
			}
			o += "\t"; o += h->pool + t.tfo_off; o += "\t"; o += h->pool + t.tts_off;
		}
		if (record_name) { o += "\t"; o += record_name; }
		o += "\n";
	}
	return text_out(o, text, text_len);
}
