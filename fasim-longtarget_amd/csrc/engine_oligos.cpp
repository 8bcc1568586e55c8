// fasim-longtarget_amd/csrc/engine_oligos.cpp -- fasim_scan_oligos: sites and potential tracks of a panel of short oligos (1 .. 112 nt)
// against a record set, and the panel table.
//
// A panel is many queries against one encoded batch and never reaches stage 3, so a work item here is a BATCH, not a (query, batch)
// pair: the worker stages and encodes the batch once (batch_encode, the head of scan_batch) and then runs, per oligo, k_scan_short
// into colmax16 and the folds that the products of the call (sites, tracks, histogram: ScanProduct, engine.h) run behind k_scan, with
// their host merges.  The engine's own query is not involved.
// fasim_scan_oligos_aligned: the same call for sites, then the hit of every site (run_site_align with k_site_ends_short, section 18).
// fasim_scan_oligos_profile / fasim_scan_oligos_peaks: the same call with k_scan_short_rows and k_rowfold_parts behind it for the
// per-base profiles, and with k_track's peak variant for the screen (section 24).
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
	const bool rows = any_rowmax(P.folds);       // a product of the call wants the row maxima: k_scan_short_rows
	for (int q = 0; q < P.nq; q++) {
		ScanShortLaunch L;
		L.tcodes = E->tcodes.as<uint8_t>(); L.unit_len = E->unit_len.as<int32_t>(); L.nunit = B.nunit; L.tstride = B.tstride;
		L.qcodes = E->oligo_q.as<uint8_t>() + (size_t)q * FASIM_MAX_OLIGO; L.m = P.m[(size_t)q]; L.colmax16 = E->colmax16.as<uint16_t>();
		scan_short_shape(L.m, B.tstride, B.nunit, &L.stretch, &L.npairs, &L.warm);
		L.rowpart16 = nullptr;
		if (rows) {
			HIPOK(E->rowpart16.ensure((size_t)B.nunit * L.npairs * (16 * ((L.m + 15) / 16)) * sizeof(uint16_t)));
			L.rowpart16 = E->rowpart16.as<uint16_t>();
		}
		hipError_t he;
		{ TimedScope ts(E, 0, E->st); he = launch_scan_short(L, E->st); }
		if (he != hipSuccess) return fail(E, FASIM_E_HIP, "scan_short launch failed: %s", hipGetErrorString(he));
		for (const ScanProduct* x : P.folds) { const int rc = x->fold(E, C, q); if (rc) return rc; }
		HIPOK(hipStreamSynchronize(E->st));      // the folds' copies are complete; colmax16 is free for the next oligo
		try { for (ScanProduct* x : P.merges) x->merge(C, *P.T, b0, b1, q); } catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	}
	return FASIM_OK;
}

// what the profile and the peaks calls add to the outputs of scan_oligos_core: profiles per oligo, or per (oligo, record), and the
// peaks of k_track per (oligo, record, class)
struct PanelExtra { int32_t per_record = 0; fasim_tfo_profile** profiles = nullptr; fasim_peak* peaks = nullptr; };

// fasim_scan_oligos, fasim_scan_oligos_hist and fasim_scan_oligos_site_counts: sites, tracks, histograms (out_hists[q]) and site counts
// (out_counts[q]) are each wanted iff their output is given, and so are the profiles and peaks of `extra`; with peaks and no tracks
// k_track runs for its peaks alone (bin 0);
// `rs` hands the resolved record set to the second phase of fasim_scan_oligos_aligned
int scan_oligos_core(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, int32_t bin, fasim_track** out_tracks, fasim_hist** out_hists, fasim_site_counts** out_counts, fasim_scan_stats* totals, RecordSet& rs, const PanelExtra& extra = PanelExtra())
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nq < 1) return fail(E, FASIM_E_ARG, "a panel needs at least one oligo (nq = %d)", nq);
	if (!oligos || !lens || !pp) return fail(E, FASIM_E_ARG, "bad arguments");
	for (int32_t q = 0; q < nq; q++) {
		if (!oligos[q] || lens[q] < 1) return fail(E, FASIM_E_ARG, "oligo %d is empty", q);
		if (lens[q] > FASIM_MAX_OLIGO)
			return fail(E, FASIM_E_ARG, "oligo %d has %d nt, a panel takes oligos of at most %d nt: scan longer queries with fasim_scan_records_sites", q, lens[q], FASIM_MAX_OLIGO);
	}
	fasim_tfo_profile** out_profiles = extra.profiles; fasim_peak* out_peaks = extra.peaks;
	if (!out_sites && !out_tracks && !out_hists && !out_counts && !out_profiles && !out_peaks) return fail(E, FASIM_E_ARG, "neither sites nor tracks are wanted");
	if (out_sites && (min_value < 1 || min_value > 16383)) return fail(E, FASIM_E_ARG, "oligos: min_value %d lies outside [1, 16383]", min_value);
	if (out_sites && max_gap < 0) return fail(E, FASIM_E_ARG, "oligos: max_gap %d is negative", max_gap);
	if (out_tracks && bin < 1) return fail(E, FASIM_E_ARG, "oligos: track bin width %d: must be at least 1", bin);
	int rc = record_set_open(E, dna, rec_off, rec_len, nrec, true, rs); if (rc) return rc;
	if (pp->cutLength <= 0 || pp->cutLength - pp->overlapLength <= 0) return fail(E, FASIM_E_ARG, "cutLength/overlapLength invalid");
	rc = record_set_bounds(E, rs); if (rc) return rc;
	rec_off = rs.rec_off; rec_len = rs.rec_len;
	const bool resident = rs.resident;
	if (pp->classicSim) return fail(E, FASIM_E_UNSUPPORTED, "oligo panels are not available with classicSim (-F): that path has no stage-2 column maxima");
	if (out_hists && 2 * (int64_t)pp->overlapLength > (int64_t)pp->cutLength)
		return fail(E, FASIM_E_UNSUPPORTED, "histograms of the potential need overlapLength (%d) of at most half of cutLength (%d): a base would lie in three segments", pp->overlapLength, pp->cutLength);
	if (out_counts && 2 * (int64_t)pp->overlapLength > (int64_t)pp->cutLength)
		return fail(E, FASIM_E_UNSUPPORTED, "site counts need overlapLength (%d) of at most half of cutLength (%d): a base would lie in three segments", pp->overlapLength, pp->cutLength);
	dna = rs.host(E);
	const fasim_params p = *pp;
	const size_t nout = (size_t)nq * (size_t)nrec;
	if (out_sites) for (size_t o = 0; o < nout; o++) out_sites[o] = nullptr;
	if (out_tracks) for (size_t o = 0; o < nout; o++) out_tracks[o] = nullptr;
	if (out_hists) for (int q = 0; q < nq; q++) out_hists[q] = nullptr;
	if (out_counts) for (int q = 0; q < nq; q++) out_counts[q] = nullptr;
	const size_t nprof = out_profiles ? (extra.per_record ? nout : (size_t)nq) : 0;
	for (size_t o = 0; o < nprof; o++) out_profiles[o] = nullptr;
	HIPOK(hipSetDevice(E->device));
	const double t_begin = now_s();
	AffinityScope numa(E->device, E->opt_numa != 0);

	// the segment table of the selected range of the global segment list, as fasim_scan_records cuts it
	const SegPlan plan = segment_plan(rec_off, rec_len, nrec, seg_first, seg_count, p);
	const SegTable& T = plan.T;
	seg_count = plan.seg_count;
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
	if (out_sites) { sites_req_init(sr, min_value, max_gap, true, nq, nrec); P.folds.push_back(&sr); }
	HistReq hr; SiteCountsReq cr; OligoTfoReq pf;
	auto drop = [&]() {
		for (size_t o = 0; o < nprof; o++) { fasim_tfo_profile_free(out_profiles[o]); out_profiles[o] = nullptr; }
		if (out_counts) for (int q = 0; q < nq; q++) { fasim_site_counts_free(out_counts[q]); out_counts[q] = nullptr; }
		if (out_hists) for (int q = 0; q < nq; q++) { fasim_hist_free(out_hists[q]); out_hists[q] = nullptr; }
		sites_drop(out_sites, nout);
		tracks_drop(out_tracks, nout);
	};
	if (out_tracks || out_peaks) {
		rc = track_req_init(E, tr, out_tracks ? bin : 0, true, nq, rec_len, nrec, out_tracks, out_peaks); if (rc) return rc;
		P.folds.push_back(&tr);
	}
	if (out_profiles) {
		pf.only = true; pf.per_record = extra.per_record != 0; pf.nrec = nrec; pf.m = P.m;
		pf.units.assign(nprof, 0); pf.sat.assign(nprof, 0); pf.mu.reset(new std::mutex[(size_t)nq]);
		pf.v.reserve(nprof * 4);
		for (size_t o = 0; o < nprof; o++) {
			out_profiles[o] = tfo_profile_alloc(P.m[extra.per_record ? o / (size_t)nrec : o]);
			if (!out_profiles[o]) { drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) pf.v.push_back(out_profiles[o]->v[c]);
		}
		P.folds.push_back(&pf); P.merges.push_back(&pf);
	}

	if (out_hists) {
		bool ok = false;
		try { ok = hist_req_init(hr, out_hists, nq, lens, rec_len, nrec, p, true); } catch (const std::bad_alloc&) { ok = false; }
		if (!ok) { for (int q = 0; q < nq; q++) out_hists[q] = nullptr; drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
		P.folds.push_back(&hr); P.merges.push_back(&hr);
	}
	if (out_counts) {
		bool ok = false;
		try { ok = site_counts_req_init(cr, out_counts, nq, lens, rec_len, nrec, p, true); } catch (const std::bad_alloc&) { ok = false; }
		if (!ok) { for (int q = 0; q < nq; q++) out_counts[q] = nullptr; drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
		P.folds.push_back(&cr); P.merges.push_back(&cr);
	}
	if (out_sites) P.merges.push_back(&sr);
	if (out_tracks || out_peaks) P.merges.push_back(&tr);
	P.T = &T;

	std::vector<int64_t> rec_units((size_t)nrec, 0);      // units scanned per record (the same for every oligo)
	fasim_scan_stats all; memset(&all, 0, sizeof all);
	if (seg_count > 0 && nenc > 0) {
		const uint8_t* dna_dev = resident ? E->dna_res.as<uint8_t>() : nullptr;
		int nworkers = workers_wanted(E);
		// batches: cut by bases as the record sets of fasim_scan_records are (at most 512 x 48 units, the bases of 384 full segments,
		// lowered so that every worker gets one; no tile rule: an oligo is one tile, and the worker target is not divided by the
		// oligos: a batch serves them all); seg_batch / FASIM_SEG_BATCH give a fixed number of segments instead
		Chunks chunks;
		const int64_t seg_batch = seg_batch_given(E);
		if (seg_batch > 0) chunks = cut_fixed(seg_count, seg_batch, 0);
		else {
			const int64_t cap = std::max<int64_t>(1, std::min<int64_t>((int64_t)512 * 48 / nenc, ((int64_t)8 << 30) / ((int64_t)4 * nenc * tstride)));
			const int64_t target = std::max<int64_t>(1, std::min<int64_t>((int64_t)384 * p.cutLength, (plan.total_bases + nworkers - 1) / nworkers));
			chunks = cut_by_bases(T, seg_count, cap, target);
		}
		nworkers = (int)std::min<size_t>((size_t)nworkers, chunks.size());
		std::vector<fasim_engine*> ws;
		rc = worker_set(E, nworkers, ws); if (rc) { drop(); return rc; }
		for (fasim_engine* w : ws) {
			rc = worker_begin(E, w, encs);
			if (!rc) { rc = upload(w, w->oligo_q, P.codes.data(), P.codes.size()); if (rc && w != E) E->err = w->err; }
			if (rc) { drop(); return rc; }
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
				worker_item_end(w, ist[c]);
				if (!r) for (int s = 0; s < ctx.nseg; s++) wunits[wi][(size_t)ctx.srec[(size_t)s]] += nenc;
				if (r) wrc[wi] = r;
			}
		};
		if (ws.size() == 1) run(0);
		else { std::vector<std::thread> th; for (size_t wi = 0; wi < ws.size(); wi++) th.emplace_back(run, wi); for (auto& t : th) t.join(); }
		rc = workers_result(E, ws, wrc); if (rc) { drop(); return rc; }
		for (size_t wi = 0; wi < ws.size(); wi++) for (int r = 0; r < nrec; r++) rec_units[(size_t)r] += wunits[wi][(size_t)r];
		for (const fasim_scan_stats& x : ist) {
			all.segments += x.segments; all.segments_skipped += x.segments_skipped; all.units += x.units;
			all.logical_cells += x.logical_cells; all.cells_stage2 += x.cells_stage2;
			for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { all.kernel_ms[k] += x.kernel_ms[k]; all.kernel_launches[k] += x.kernel_launches[k]; }
		}
	}

	if (out_sites) {
		// the kernel's runs of one (oligo, record), united and joined by the sweep every site list goes through
		rc = sites_req_finish(E, sr, out_sites, [&](size_t o) { return rec_units[o % (size_t)nrec]; });
		if (rc) { drop(); return rc; }
	}
	if (out_tracks) for (size_t o = 0; o < nout; o++) { out_tracks[o]->units = rec_units[o % (size_t)nrec]; out_tracks[o]->saturated_units = tr.sat[o]; }
	for (size_t o = 0; o < nprof; o++) { out_profiles[o]->units = pf.units[o]; out_profiles[o]->saturated_units = pf.sat[o]; }
	if (out_hists) {
		try { rc = hist_req_finish(E, hr, out_hists, nq); } catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
		if (rc) { drop(); return rc; }
	}
	if (out_counts) {
		try { rc = site_counts_req_finish(E, cr, out_counts, nq); } catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
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

// k_rowfold_parts over the parts k_scan_short_rows left of oligo q in E->rowpart16, into C.rowfold: the groups are TfoReq::fold's, one
// per run of segments of one record, or the whole batch.  The shape of the parts is the one panel_batch launched the scan with.  The
// copy completes at the next synchronisation of the stream; TfoReq::merge then takes C.rowfold as k_rowfold's.
int OligoTfoReq::fold(fasim_engine* E, BatchCtx& C, int q) const
{
	const int nu = C.B.nunit, nseg = C.nseg, mq = m[(size_t)q], rows = 16 * ((mq + 15) / 16);
	int rc; hipError_t he;
	std::vector<int32_t>& gfirst = C.row_gfirst;
	gfirst.assign(1, 0);
	if (per_record) for (int s = 1; s < nseg; s++) if (C.srec[(size_t)s] != C.srec[(size_t)s - 1]) gfirst.push_back(s);
	gfirst.push_back(nseg);
	const int ng = (int)gfirst.size() - 1;
	const size_t nout = (size_t)ng * 4 * rows;
	rc = upload(E, E->row_gfirst, gfirst.data(), sizeof(int32_t) * gfirst.size()); if (rc) return rc;
	HIPOK(E->row_out.ensure(nout * sizeof(uint16_t)));
	RowPartFoldLaunch R;
	int warm;
	scan_short_shape(mq, C.B.tstride, nu, &R.stretch, &R.npairs, &warm);
	R.rowpart16 = E->rowpart16.as<uint16_t>(); R.unit_len = E->unit_len.as<int32_t>(); R.gfirst = E->row_gfirst.as<int32_t>();
	R.ngroups = ng; R.nenc = C.nenc; R.rows = rows; R.tab = C.tab; R.out = E->row_out.as<uint16_t>();
	{ TimedScope ts(E, 4); he = launch_rowfold_parts(R, E->st); }
	if (he != hipSuccess) return fail(E, FASIM_E_HIP, "rowfold launch failed: %s", hipGetErrorString(he));
	C.rowfold.resize(nout); C.row_sat.assign((size_t)nu, 0);      // (no row maximum of an oligo saturates)
	HIPOK(hipMemcpyAsync(C.rowfold.data(), E->row_out.p, nout * sizeof(uint16_t), hipMemcpyDeviceToHost, E->st));
	return FASIM_OK;
}

extern "C" {

int fasim_scan_oligos_profile(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t per_record, fasim_tfo_profile** out_profiles, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_profiles) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	PanelExtra x; x.per_record = per_record; x.profiles = out_profiles;
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, 1, 0, nullptr, 1, nullptr, nullptr, nullptr, totals, rs, x);
}

int fasim_scan_oligos_peaks(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t bin, fasim_track** out_tracks, fasim_peak* out_peaks, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_peaks) return fail(E, FASIM_E_ARG, "bad arguments");
	if (bin < 0) return fail(E, FASIM_E_ARG, "oligos: track bin width %d: must be at least 1, or 0 for peaks only", bin);
	if (bin == 0 && out_tracks) return fail(E, FASIM_E_ARG, "oligos: bin 0 is peaks only: out_tracks must be NULL");
	if (bin >= 1 && !out_tracks) return fail(E, FASIM_E_ARG, "oligos: bin %d needs out_tracks", bin);
	RecordSet rs;
	PanelExtra x; x.peaks = out_peaks;
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, 1, 0, nullptr, bin, out_tracks, nullptr, nullptr, totals, rs, x);
}

int fasim_scan_oligos(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, int32_t bin, fasim_track** out_tracks, fasim_scan_stats* totals)
{
	RecordSet rs;
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_sites, bin, out_tracks, nullptr, nullptr, totals, rs);
}

int fasim_scan_oligos_aligned(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_sites** out_sites, fasim_site_hits** out_hits, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_sites || !out_hits) return fail(E, FASIM_E_ARG, "bad arguments");
	// first phase: the sites call itself, refusals included (its sites and totals are this call's)
	RecordSet rs;
	int rc = scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_sites, 1, nullptr, nullptr, nullptr, totals, rs);
	if (rc) return rc;
	const size_t nout = (size_t)nq * (size_t)nrec;
	for (size_t o = 0; o < nout; o++) out_hits[o] = nullptr;
	// second phase: the hits, oligo by oligo, on the engine's own stream (section 18)
	SiteAlignReq R;
	R.dna = rs.host(E); R.rec_off = rs.rec_off; R.rec_len = rs.rec_len; R.nrec = nrec; R.seg_first = seg_first; R.seg_count = seg_count;
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
	RecordSet rs;
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, 1, 0, nullptr, 1, nullptr, out_hists, nullptr, totals, rs);
}

int fasim_scan_oligos_site_counts(fasim_engine* E, const char* const* oligos, const int32_t* lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_site_counts** out_counts, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_counts) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	return scan_oligos_core(E, oligos, lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, 1, 0, nullptr, 1, nullptr, nullptr, out_counts, totals, rs);
}

int fasim_oligo_panel_tsv(const char* const* names, const int32_t* lens, int32_t nq, const fasim_sites* const* sites, int32_t nrec,
	char** text, int64_t* text_len)
{
	if (!names || !lens || nq < 0 || nrec < 0 || !text || !text_len || (nq > 0 && nrec > 0 && !sites)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "oligo\tlength\ttotal_sites\tcovered_bases";
	for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "_sites\t"; o += c; o += "_max"; }
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
