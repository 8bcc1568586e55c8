// fasim-longtarget_amd/csrc/engine_oligos.cpp -- fasim_scan_oligos: sites and potential tracks of a panel of short oligos (1 .. 112 nt)
// against a record set, and the panel table.
//
// A panel is many queries against one encoded batch and never reaches stage 3, so a work item here is a BATCH, not a (query, batch)
// pair: the worker stages and encodes the batch once (batch_encode, the head of scan_batch) and then runs, per oligo, k_scan_short
// into colmax16 and the folds that the products of the call (sites, tracks, histogram: ScanProduct, engine.h) run behind k_scan, with
// their host merges.  The engine's own query is not involved.
// fasim_scan_oligos_aligned: the same call for sites, then the hit of every site (run_site_align with k_site_ends_short, section 18).
#include "engine.h"

namespace {

// what one call shares with its workers
struct PanelCall {
	int nq = 0, nrec = 0, tstride = 0;
	std::vector<int32_t> m;                      // [oligo]
	std::vector<uint8_t> codes;                  // [oligo][FASIM_MAX_OLIGO], stage-2 alphabet
	ScanProducts folds, merges;                  // the products wanted, in the order of their folds and of their merges
	const SegTable* T = nullptr;
};

// one batch on one worker: `C` comes from batch_encode, the batch's target codes are in w->tcodes
int panel_batch(fasim_engine* E, const PanelCall& P, BatchCtx& C, int64_t b0, int64_t b1)
{
	const UnitBatch& B = C.B;
	HIPOK(E->colmax16.ensure((size_t)B.nunit * B.tstride * sizeof(uint16_t)));
	for (int q = 0; q < P.nq; q++) {
		ScanShortLaunch L;
		L.tcodes = E->tcodes.as<uint8_t>(); L.unit_len = E->unit_len.as<int32_t>(); L.nunit = B.nunit; L.tstride = B.tstride;
		L.qcodes = E->oligo_q.as<uint8_t>() + (size_t)q * FASIM_MAX_OLIGO; L.m = P.m[(size_t)q]; L.colmax16 = E->colmax16.as<uint16_t>();
		scan_short_shape(L.m, B.tstride, B.nunit, &L.stretch, &L.npairs, &L.warm);
		hipError_t he;
		{ TimedScope ts(E, 0, E->st); he = launch_scan_short(L, E->st); }
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "scan_short launch failed: %s", hipGetErrorString(he));
		for (const ScanProduct* x : P.folds) { const int rc = x->fold(E, C, q); if (rc) return rc; }
		HIPOK(hipStreamSynchronize(E->st));      // the folds' copies are complete; colmax16 is free for the next oligo
		try { for (ScanProduct* x : P.merges) x->merge(C, *P.T, b0, b1, q); } catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	}
	return FASIM_OK;
}

// fasim_scan_oligos and fasim_scan_oligos_hist: sites, tracks and histograms (out_hists[q]) are each wanted iff their output is given
int scan_oligos_core(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, int32_t bin, fasim_track** out_tracks, fasim_hist** out_hists, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nq < 1) return fail(E, FASIM_E_ARG, "a panel needs at least one oligo (nq = %d)", nq);
	if (!oligos || !lens || !pp) return fail(E, FASIM_E_ARG, "bad arguments");
	for (int32_t q = 0; q < nq; q++) {
		if (!oligos[q] || lens[q] < 1) return fail(E, FASIM_E_ARG, "oligo %d is empty", q);
		if (lens[q] > FASIM_MAX_OLIGO)
			return fail(E, FASIM_E_ARG, "oligo %d has %d nt, a panel takes oligos of at most %d nt: scan longer queries with fasim_scan_records_sites", q, lens[q], FASIM_MAX_OLIGO);
	}
	if (!out_sites && !out_tracks && !out_hists) return fail(E, FASIM_E_ARG, "neither sites nor tracks are wanted");
	if (out_sites && (min_value < 1 || min_value > 16383)) return fail(E, FASIM_E_ARG, "oligos: min_value %d lies outside [1, 16383]", min_value);
	if (out_sites && max_gap < 0) return fail(E, FASIM_E_ARG, "oligos: max_gap %d is negative", max_gap);
	if (out_tracks && bin < 1) return fail(E, FASIM_E_ARG, "oligos: track bin width %d: must be at least 1", bin);
	const int64_t whole_off = 0, whole_len = (int64_t)E->dna_host.size();
	if (!dna && !rec_off && !rec_len && nrec == 1) {           // the whole resident buffer as one record
		if (whole_len == 0) return fail(E, FASIM_E_ARG, "no resident DNA: call fasim_load_dna first");
		rec_off = &whole_off; rec_len = &whole_len;
	}
	if (nrec < 1) return fail(E, FASIM_E_ARG, "a record set needs at least one record (nrec = %d)", nrec);
	if (!rec_off || !rec_len) return fail(E, FASIM_E_ARG, "bad arguments");
	if (pp->cutLength <= 0 || pp->cutLength - pp->overlapLength <= 0) return fail(E, FASIM_E_ARG, "cutLength/overlapLength invalid");
	const bool resident = dna == nullptr;
	if (resident && E->dna_host.empty()) return fail(E, FASIM_E_ARG, "no resident DNA: call fasim_load_dna first");
	{
		const int64_t have = resident ? (int64_t)E->dna_host.size() : INT64_MAX;
		for (int32_t r = 0; r < nrec; r++) {
			if (rec_len[r] == 0) return fail(E, FASIM_E_ARG, "record %d is empty", r);
			if (rec_off[r] < 0 || rec_len[r] < 0 || rec_off[r] > have || rec_len[r] > have - rec_off[r])
				return fail(E, FASIM_E_ARG, "record %d: offset %lld, length %lld lies outside the DNA buffer%s", r, (long long)rec_off[r],
					(long long)rec_len[r], resident ? " (the resident buffer of fasim_load_dna)" : "");
			if (rec_len[r] > 0x7fffffffll) return fail(E, FASIM_E_ARG, "record %d: one record is limited to 2^31-1 nt (the reference's int positions)", r);
		}
	}
	if (pp->classicSim) return fail(E, FASIM_E_UNSUPPORTED, "oligo panels are not available with classicSim (-F): that path has no stage-2 column maxima");
	if (out_hists && 2 * (int64_t)pp->overlapLength > (int64_t)pp->cutLength)
		return fail(E, FASIM_E_UNSUPPORTED, "histograms of the potential need overlapLength (%d) of at most half of cutLength (%d): a base would lie in three segments", pp->overlapLength, pp->cutLength);
	if (resident) dna = E->dna_host.data();
	const fasim_params p = *pp;
	const size_t nout = (size_t)nq * (size_t)nrec;
	if (out_sites) for (size_t o = 0; o < nout; o++) out_sites[o] = nullptr;
	if (out_tracks) for (size_t o = 0; o < nout; o++) out_tracks[o] = nullptr;
	if (out_hists) for (int q = 0; q < nq; q++) out_hists[q] = nullptr;
	HIPOK(hipSetDevice(E->device));
	const double t_begin = now_s();
	AffinityScope numa(E->device, E->opt_numa != 0);

	// the segment table of the selected range of the global segment list, as fasim_scan_records cuts it
	const int64_t step = p.cutLength - p.overlapLength;
	std::vector<int64_t> rec_first((size_t)nrec + 1, 0);
	for (int r = 0; r < nrec; r++) rec_first[(size_t)r + 1] = rec_first[(size_t)r] + fasim_segment_count(rec_len[r], &p);
	const int64_t nseg_all = rec_first[(size_t)nrec];
	if (seg_first < 0) seg_first = 0;
	if (seg_count < 0 || seg_first + seg_count > nseg_all) seg_count = std::max<int64_t>(0, nseg_all - seg_first);
	SegTable T;
	int64_t total_bases = 0;
	if (seg_count > 0) {
		int r = (int)(std::upper_bound(rec_first.begin(), rec_first.end(), seg_first) - rec_first.begin()) - 1;
		for (int64_t g = seg_first; g < seg_first + seg_count; g++) {
			while (g >= rec_first[(size_t)r + 1]) r++;
			const int64_t i = g - rec_first[(size_t)r], pos = i * step;
			const int len = (int)std::min<int64_t>(p.cutLength, rec_len[r] - pos);
			T.rec.push_back(r); T.idx.push_back(i); T.off.push_back(rec_off[r] + pos); T.len.push_back(len);
			total_bases += len;
		}
	}
	const std::vector<int> encs = enabled_encodings(p);
	const int nenc = (int)encs.size();
	const int tstride = (p.cutLength + 15) & ~15;

	PanelCall P;
	P.nq = nq; P.nrec = nrec; P.tstride = tstride;
	P.m.assign(lens, lens + nq);
	P.codes.assign((size_t)nq * FASIM_MAX_OLIGO, 4);
	int64_t msum = 0;
	for (int q = 0; q < nq; q++) { msum += lens[q]; for (int i = 0; i < lens[q]; i++) P.codes[(size_t)q * FASIM_MAX_OLIGO + i] = code2(oligos[q][i]); }
	SitesReq sr; TrackReq tr;
	if (out_sites) {
		sr.min_value = min_value; sr.max_gap = max_gap; sr.only = true; sr.nrec = nrec;
		sr.runs.resize(nout); sr.sat.assign(nout, 0); sr.mu.reset(new std::mutex[(size_t)nq]);
		P.folds.push_back(&sr);
	}
	HistReq hr;
	auto drop = [&]() {
		if (out_hists) for (int q = 0; q < nq; q++) { fasim_hist_free(out_hists[q]); out_hists[q] = nullptr; }
		if (out_sites) for (size_t o = 0; o < nout; o++) { fasim_sites_free(out_sites[o]); out_sites[o] = nullptr; }
		if (out_tracks) for (size_t o = 0; o < nout; o++) { fasim_track_free(out_tracks[o]); out_tracks[o] = nullptr; }
	};
	if (out_tracks) {
		tr.bin = bin; tr.only = true; tr.nrec = nrec; tr.sat.assign(nout, 0); tr.mu.reset(new std::mutex[(size_t)nq]);
		tr.nbins.resize((size_t)nrec);
		for (int r = 0; r < nrec; r++) tr.nbins[(size_t)r] = (rec_len[r] + bin - 1) / bin;
		tr.v.reserve(nout * 4);
		for (size_t o = 0; o < nout; o++) {
			out_tracks[o] = track_alloc(tr.nbins[o % (size_t)nrec], bin);
			if (!out_tracks[o]) { drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) tr.v.push_back(out_tracks[o]->v[c]);
		}
		P.folds.push_back(&tr);
	}

	if (out_hists) {
		bool ok = false;
		try { ok = hist_req_init(hr, out_hists, nq, lens, rec_len, nrec, p, true); } catch (const std::bad_alloc&) { ok = false; }
		if (!ok) { for (int q = 0; q < nq; q++) out_hists[q] = nullptr; drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
		P.folds.push_back(&hr); P.merges.push_back(&hr);
	}
	if (out_sites) P.merges.push_back(&sr);
	if (out_tracks) P.merges.push_back(&tr);
	P.T = &T;

	std::vector<int64_t> rec_units((size_t)nrec, 0);      // units scanned per record (the same for every oligo)
	fasim_scan_stats all; memset(&all, 0, sizeof all);
	if (seg_count > 0 && nenc > 0) {
		const uint8_t* dna_dev = resident ? E->dna_res.as<uint8_t>() : nullptr;
		int nworkers = 10;
		const char* envw = getenv("FASIM_WORKERS");
		if (envw) nworkers = std::max(1, std::min(16, atoi(envw)));
		if (E->opt_workers > 0) nworkers = std::min(16, E->opt_workers);
		// batches: cut by bases as the record sets of fasim_scan_records are (at most 512 x 48 units, the bases of 384 full segments,
		// lowered so that every worker gets one); seg_batch / FASIM_SEG_BATCH give a fixed number of segments instead
		std::vector<std::pair<int64_t, int64_t>> chunks;
		const char* envb = getenv("FASIM_SEG_BATCH");
		int64_t seg_batch = envb ? std::max(1, atoi(envb)) : 0;
		if (E->opt_seg_batch > 0) seg_batch = E->opt_seg_batch;
		if (seg_batch > 0) {
			for (int64_t b0 = 0; b0 < seg_count; b0 += seg_batch) chunks.push_back({ b0, std::min(seg_count, b0 + seg_batch) });
		} else {
			const int64_t cap = std::max<int64_t>(1, std::min<int64_t>((int64_t)512 * 48 / nenc, ((int64_t)8 << 30) / ((int64_t)4 * nenc * tstride)));
			const int64_t target = std::max<int64_t>(1, std::min<int64_t>((int64_t)384 * p.cutLength, (total_bases + nworkers - 1) / nworkers));
			int64_t b0 = 0, bases = 0;
			for (int64_t s = 0; s < seg_count; s++) {
				bases += T.len[(size_t)s];
				if (s + 1 - b0 >= cap || bases >= target) { chunks.push_back({ b0, s + 1 }); b0 = s + 1; bases = 0; }
			}
			if (b0 < seg_count) chunks.push_back({ b0, seg_count });
		}
		nworkers = (int)std::min<size_t>((size_t)nworkers, chunks.size());
		while ((int)E->workers.size() < nworkers - 1) {
			fasim_engine* w = nullptr;
			int rc = fasim_engine_create(E->device, &w); if (rc) { drop(); return fail(E, rc, "cannot create worker engine: %s", fasim_last_error(nullptr)); }
			E->workers.push_back(w);
		}
		std::vector<fasim_engine*> ws(1, E);
		for (int k = 0; k < nworkers - 1; k++) ws.push_back(E->workers[(size_t)k]);
		for (fasim_engine* w : ws) {
			int rc = upload(w, w->enc_ids, encs.data(), sizeof(int) * nenc);
			if (!rc) rc = upload(w, w->oligo_q, P.codes.data(), P.codes.size());
			if (rc) { if (w != E) E->err = w->err; drop(); return rc; }
			drain_timed(w);
			for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { w->kernel_ms[k] = 0; w->kernel_launches[k] = 0; }
		}
		std::vector<fasim_scan_stats> ist(chunks.size());
		for (auto& x : ist) memset(&x, 0, sizeof x);
		std::vector<int> wrc(ws.size(), FASIM_OK);
		std::vector<std::vector<int64_t>> wunits(ws.size(), std::vector<int64_t>((size_t)nrec, 0));
		std::atomic<size_t> next(0);
		auto run = [&](size_t wi) {
			(void)hipSetDevice(E->device);
			fasim_engine* w = ws[wi];
			for (;;) {
				const size_t c = next.fetch_add(1);
				if (c >= chunks.size() || wrc[wi]) break;
				BatchCtx ctx;
				int r = batch_encode(w, dna, T, dna_dev, chunks[c].first, chunks[c].second, p, encs, tstride, ctx, ist[c], msum);
				if (!r && ctx.nseg > 0) r = panel_batch(w, P, ctx, chunks[c].first, chunks[c].second);
				else if (!r) {
					// (a batch whose segments are all skipped still has positions for the histogram to count: they lie in bin 0)
					try { for (ScanProduct* x : P.merges) if (x->merges_empty()) for (int q = 0; q < nq; q++) x->merge(ctx, T, chunks[c].first, chunks[c].second, q); }
					catch (const std::bad_alloc&) { r = fail(w, FASIM_E_NOMEM, "out of memory"); }
				}
				(void)hipStreamSynchronize(w->st);
				drain_timed(w);
				for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { ist[c].kernel_ms[k] = w->kernel_ms[k]; ist[c].kernel_launches[k] = w->kernel_launches[k]; w->kernel_ms[k] = 0; w->kernel_launches[k] = 0; }
				if (!r) for (int s = 0; s < ctx.nseg; s++) wunits[wi][(size_t)ctx.srec[(size_t)s]] += nenc;
				if (r) wrc[wi] = r;
			}
		};
		if (ws.size() == 1) run(0);
		else { std::vector<std::thread> th; for (size_t wi = 0; wi < ws.size(); wi++) th.emplace_back(run, wi); for (auto& t : th) t.join(); }
		for (size_t wi = 0; wi < ws.size(); wi++) if (wrc[wi]) { if (ws[wi] != E) E->err = ws[wi]->err; drop(); return wrc[wi]; }
		for (size_t wi = 0; wi < ws.size(); wi++) for (int r = 0; r < nrec; r++) rec_units[(size_t)r] += wunits[wi][(size_t)r];
		for (const fasim_scan_stats& x : ist) {
			all.segments += x.segments; all.segments_skipped += x.segments_skipped; all.units += x.units;
			all.logical_cells += x.logical_cells; all.cells_stage2 += x.cells_stage2;
			for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { all.kernel_ms[k] += x.kernel_ms[k]; all.kernel_launches[k] += x.kernel_launches[k]; }
		}
	}

	if (out_sites) {
		// the kernel's runs of one (oligo, record) as a site list of their own, united and joined by the sweep every site list goes through
		try {
			std::vector<fasim_site> v;
			for (size_t o = 0; o < nout; o++) {
				const std::vector<HostRun>& runs = sr.runs[o];
				v.clear(); v.reserve(runs.size());
				for (const HostRun& h : runs) { fasim_site x; x.start = h.start; x.end = h.end; x.pos = h.pos; x.value = h.value; x.enc = h.enc; x.cls = h.cls; x.reserved = 0; v.push_back(x); }
				fasim_sites raw; memset(&raw, 0, sizeof raw);
				raw.n = (int64_t)v.size(); raw.s = v.data(); raw.min_value = min_value; raw.max_gap = max_gap;
				raw.units = rec_units[o % (size_t)nrec]; raw.saturated_units = sr.sat[o]; raw.raw_runs = (int64_t)runs.size();
				const fasim_sites* part = &raw;
				const int rc = fasim_sites_merge(&part, 1, &out_sites[o]);
				if (rc) { drop(); return fail(E, rc, "%s", fasim_last_error(nullptr)); }
			}
		} catch (const std::bad_alloc&) { drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	}
	if (out_tracks) for (size_t o = 0; o < nout; o++) { out_tracks[o]->units = rec_units[o % (size_t)nrec]; out_tracks[o]->saturated_units = tr.sat[o]; }
	if (out_hists) {
		int rc;
		try { rc = hist_req_finish(E, hr, out_hists, nq); } catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
		if (rc) { drop(); return rc; }
	}
	if (totals) {
		const double t_total = now_s() - t_begin;
		for (int q = 0; q < nq; q++) {
			fasim_scan_stats& x = totals[q];
			memset(&x, 0, sizeof x);
			x.segments = all.segments; x.segments_skipped = all.segments_skipped; x.units = all.units;
			x.logical_cells = msum ? all.logical_cells / msum * lens[q] : 0; x.cells_stage2 = msum ? all.cells_stage2 / msum * lens[q] : 0;
			for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { x.kernel_ms[k] = all.kernel_ms[k] / nq; x.kernel_launches[k] = all.kernel_launches[k] / nq; }
			x.t_total_s = t_total;
		}
	}
	return FASIM_OK;
}

} // namespace

extern "C" {

int fasim_scan_oligos(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, int32_t bin, fasim_track** out_tracks, fasim_scan_stats* totals)
{
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_sites, bin, out_tracks, nullptr, totals);
}

int fasim_scan_oligos_aligned(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, fasim_site_hits** out_hits, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_sites || !out_hits) return fail(E, FASIM_E_ARG, "bad arguments");
	// first phase: the sites call itself, refusals included (its sites and totals are this call's)
	int rc = scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_sites, 1, nullptr, nullptr, totals);
	if (rc) return rc;
	const size_t nout = (size_t)nq * (size_t)nrec;
	for (size_t o = 0; o < nout; o++) out_hits[o] = nullptr;
	const int64_t whole_off = 0, whole_len = (int64_t)E->dna_host.size();
	if (!dna && !rec_off && !rec_len && nrec == 1) { rec_off = &whole_off; rec_len = &whole_len; }
	// second phase: the hits, oligo by oligo, on the engine's own stream (section 18)
	SiteAlignReq R;
	R.dna = dna ? dna : E->dna_host.data(); R.rec_off = rec_off; R.rec_len = rec_len; R.nrec = nrec; R.seg_first = seg_first; R.seg_count = seg_count;
	R.p = *pp; R.sites = out_sites; R.hits = out_hits; R.short_query = site_short_enabled(E);
	try {
		for (int q = 0; q < nq; q++) R.queries.emplace_back(oligos[q], oligos[q] + lens[q]);
		rc = run_site_align(E, R);
	} catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (rc) {
		(void)hipStreamSynchronize(E->st);
		for (size_t o = 0; o < nout; o++) {
			site_hits_free(out_hits[o]); out_hits[o] = nullptr;
			fasim_sites_free(out_sites[o]); out_sites[o] = nullptr;
		}
	}
	return rc;
}

int fasim_scan_oligos_hist(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_hist** out_hists, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_hists) return fail(E, FASIM_E_ARG, "bad arguments");
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, 1, 0, nullptr, 1, nullptr, out_hists, totals);
}

int fasim_oligo_panel_tsv(const char* const* names, const int32_t* lens, int32_t nq, const fasim_sites* const* sites, int32_t nrec,
	char** text, int64_t* text_len)
{
	if (!names || !lens || nq < 0 || nrec < 0 || !text || !text_len || (nq > 0 && nrec > 0 && !sites)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	static const char* const cls_names[FASIM_TRACK_CLASSES] = { "ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus" };
	std::string o = "oligo\tlength\ttotal_sites\tcovered_bases";
	for (const char* c : cls_names) { o += "\t"; o += c; o += "_sites\t"; o += c; o += "_max"; }
	o += "\n";
	for (int32_t q = 0; q < nq; q++) {
		if (!names[q]) return fail(nullptr, FASIM_E_ARG, "oligo %d has no name", q);
		int64_t cnt[FASIM_TRACK_CLASSES] = { 0 }, covered = 0, total = 0;
		int32_t top[FASIM_TRACK_CLASSES] = { 0 };
		for (int32_t r = 0; r < nrec; r++) {
			const fasim_sites* t = sites[(size_t)q * (size_t)nrec + (size_t)r];
			if (!t || t->n < 0 || (t->n > 0 && !t->s)) return fail(nullptr, FASIM_E_ARG, "bad site list of oligo %d, record %d", q, r);
			for (int64_t i = 0; i < t->n; i++) {
				const fasim_site& x = t->s[i];
				if (x.cls < 0 || x.cls >= FASIM_TRACK_CLASSES) return fail(nullptr, FASIM_E_ARG, "a site of oligo %d, record %d has class %d", q, r, x.cls);
				cnt[x.cls]++; total++; covered += x.end - x.start; top[x.cls] = std::max(top[x.cls], x.value);
			}
		}
		o += names[q]; o += "\t"; o += std::to_string(lens[q]); o += "\t"; o += std::to_string(total); o += "\t"; o += std::to_string(covered);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) { o += "\t"; o += std::to_string(cnt[c]); o += "\t"; o += std::to_string(top[c]); }
		o += "\n";
	}
	return text_out(o, text, text_len);
}

} // extern "C"
