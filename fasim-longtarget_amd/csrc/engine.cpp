// fasim-longtarget_amd/csrc/engine.cpp -- the C-ABI of libfasim_hip.so (include/fasim_hip.h); the engine behind it lives in
// engine.h, engine_stage2.cpp, engine_stage3.cpp and engine_scan.cpp.
#include "engine.h"

// =====================================================================================================
// The frame of a call (declared in engine.h): what the record-set entry points share before and after their scan
// =====================================================================================================
// FASIM_MAX_QUERY (fasim_hip.h): above it the reference's 16-bit stage-1 pass overruns its workspace
static int refuse_long_query(fasim_engine* E, int64_t len, int index)
{
	char which[32] = "";
	if (index >= 0) snprintf(which, sizeof which, " (query %d)", index);
	return fail(E, FASIM_E_UNSUPPORTED, "query of %lld nt%s exceeds the limit of %d nt: above it the reference's 16-bit stage-1 pass "
		"overruns its fixed workspace (stats.h:397) and its output is undefined", (long long)len, which, FASIM_MAX_QUERY);
}

int record_set_open(fasim_engine* E, const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, bool whole_ok, RecordSet& rs)
{
	rs.dna = dna; rs.rec_off = rec_off; rs.rec_len = rec_len; rs.nrec = nrec; rs.resident = dna == nullptr;
	if (whole_ok && !dna && !rec_off && !rec_len && nrec == 1) {           // the whole resident buffer as one record: the engine knows its length
		rs.whole_off = 0; rs.whole_len = (int64_t)E->dna_host.size();
		if (rs.whole_len == 0) return fail(E, FASIM_E_ARG, "no resident DNA: call fasim_load_dna first");
		rs.rec_off = &rs.whole_off; rs.rec_len = &rs.whole_len;
	}
	if (nrec < 1) return fail(E, FASIM_E_ARG, "a record set needs at least one record (nrec = %d)", nrec);
	if (!rs.rec_off || !rs.rec_len) return fail(E, FASIM_E_ARG, "bad arguments");
	return FASIM_OK;
}

int record_set_bounds(fasim_engine* E, const RecordSet& rs)
{
	// a host buffer has no length here: only the resident buffer bounds the offsets from above
	if (rs.resident && E->dna_host.empty()) return fail(E, FASIM_E_ARG, "no resident DNA: call fasim_load_dna first");
	const int64_t have = rs.resident ? (int64_t)E->dna_host.size() : INT64_MAX;
	for (int32_t r = 0; r < rs.nrec; r++) {
		const int64_t off = rs.rec_off[r], len = rs.rec_len[r];
		if (len == 0) return fail(E, FASIM_E_ARG, "record %d is empty", r);
		if (off < 0 || len < 0 || off > have || len > have - off)
			return fail(E, FASIM_E_ARG, "record %d: offset %lld, length %lld lies outside the DNA buffer%s", r, (long long)off,
				(long long)len, rs.resident ? " (the resident buffer of fasim_load_dna)" : "");
		if (len > 0x7fffffffll) return fail(E, FASIM_E_ARG, "record %d: one record is limited to 2^31-1 nt (the reference's int positions)", r);
	}
	return FASIM_OK;
}

// argument checks of fasim_scan_records and the calls built on it, before any GPU work
int check_records_args(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_params* pp, bool whole_ok, RecordSet& rs)
{
	int rc = record_set_open(E, dna, rec_off, rec_len, nrec, whole_ok, rs); if (rc) return rc;
	if (!pp || nq < 0) return fail(E, FASIM_E_ARG, "bad arguments");
	if (pp->cutLength <= 0 || pp->cutLength - pp->overlapLength <= 0) return fail(E, FASIM_E_ARG, "cutLength/overlapLength invalid");
	if (nq == 0) { rc = need_query(E); if (rc) return rc; }
	else {
		if (!rnas || !rna_lens) return fail(E, FASIM_E_ARG, "bad arguments");
		for (int32_t q = 0; q < nq; q++) {
			if (!rnas[q] || rna_lens[q] <= 0) return fail(E, FASIM_E_ARG, "empty query %d", q);
			if (rna_lens[q] > FASIM_MAX_QUERY) return refuse_long_query(E, rna_lens[q], q);
		}
	}
	return record_set_bounds(E, rs);
}

// the potential is the column maxima of the systolic scan kernel: no other kernel leaves them
int check_track_source(fasim_engine* E, const int32_t* rna_lens, int32_t nq, const fasim_params* pp, const char* what)
{
	for (int q = 0; q < std::max(1, nq); q++) {
		const int len = nq == 0 ? E->m : rna_lens[q];
		if (!systolic_fits(len)) return fail(E, FASIM_E_UNSUPPORTED, "%s need a query of at least 113 nt (query %d has %d): shorter queries run on the striped kernels, which keep the reference's 8-bit column maxima only", what, q, len);
	}
	if (E->scan_v1) return fail(E, FASIM_E_UNSUPPORTED, "%s are not available under FASIM_SCAN_V1=1 (the striped kernels keep the reference's 8-bit column maxima only)", what);
	if (pp->classicSim) return fail(E, FASIM_E_UNSUPPORTED, "%s are not available with classicSim (-F): that path has no stage-2 column maxima", what);
	return FASIM_OK;
}

int workers_wanted(const fasim_engine* E)
{
	int nworkers = 10;
	const char* envw = getenv("FASIM_WORKERS");
	if (envw) nworkers = std::max(1, std::min(16, atoi(envw)));
	if (E->opt_workers > 0) nworkers = std::min(16, E->opt_workers);
	return nworkers;
}

int64_t seg_batch_given(const fasim_engine* E)
{
	const char* envb = getenv("FASIM_SEG_BATCH");
	int64_t seg_batch = envb ? std::max(1, atoi(envb)) : 0;
	if (E->opt_seg_batch > 0) seg_batch = E->opt_seg_batch;
	return seg_batch;
}

int worker_set(fasim_engine* E, int wanted, std::vector<fasim_engine*>& ws)
{
	// worker 0 is this engine; the others are lazily created engines on the same device
	while ((int)E->workers.size() < wanted - 1) {
		fasim_engine* w = nullptr;
		const int rc = fasim_engine_create(E->device, &w); if (rc) return fail(E, rc, "cannot create worker engine: %s", fasim_last_error(nullptr));
		E->workers.push_back(w);
	}
	ws.assign(1, E);
	for (int k = 0; k < wanted - 1; k++) ws.push_back(E->workers[(size_t)k]);
	return FASIM_OK;
}

int worker_begin(fasim_engine* E, fasim_engine* w, const std::vector<int>& encs)
{
	HIPOK(hipSetDevice(E->device));
	const int rc = upload(w, w->enc_ids, encs.data(), sizeof(int) * encs.size());
	if (rc) { if (w != E) E->err = w->err; return rc; }
	drain_timed(w);
	for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { w->kernel_ms[k] = 0; w->kernel_launches[k] = 0; }
	w->sw_probs = 0; w->sw_ms = 0.0;
	return FASIM_OK;
}

void worker_item_end(fasim_engine* w, fasim_scan_stats& st)
{
	(void)hipStreamSynchronize(w->st);
	drain_timed(w);
	for (int k = 0; k < FASIM_KERNEL_FAMILIES; k++) { st.kernel_ms[k] = w->kernel_ms[k]; st.kernel_launches[k] = w->kernel_launches[k]; w->kernel_ms[k] = 0; w->kernel_launches[k] = 0; }
	st.striped_window_probs = w->sw_probs; st.striped_window_ms = w->sw_ms; w->sw_probs = 0; w->sw_ms = 0.0;
}

int workers_result(fasim_engine* E, const std::vector<fasim_engine*>& ws, const std::vector<int>& wrc)
{
	for (size_t wi = 0; wi < ws.size(); wi++) if (wrc[wi]) { if (ws[wi] != E) E->err = ws[wi]->err; return wrc[wi]; }
	return FASIM_OK;
}

void tracks_drop(fasim_track** out_tracks, size_t nout)
{
	if (out_tracks) for (size_t o = 0; o < nout; o++) { fasim_track_free(out_tracks[o]); out_tracks[o] = nullptr; }
}

int track_req_init(fasim_engine* E, TrackReq& tr, int32_t bin, bool only, int nquery, const int64_t* rec_len, int nrec, fasim_track** out_tracks, fasim_peak* peaks)
{
	const size_t nout = (size_t)nquery * (size_t)nrec;
	tr.bin = bin; tr.only = only; tr.nrec = nrec; tr.peaks = peaks;
	tr.sat.assign(nout, 0); tr.mu.reset(new std::mutex[(size_t)nquery]);
	if (peaks) for (size_t k = 0; k < nout * 4; k++) { peaks[k].value = 0; peaks[k].enc = -1; peaks[k].pos = -1; }
	if (bin < 1) return FASIM_OK;
	tr.nbins.resize((size_t)nrec);
	for (int r = 0; r < nrec; r++) tr.nbins[(size_t)r] = (rec_len[r] + bin - 1) / bin;
	tr.v.reserve(nout * 4);
	for (size_t o = 0; o < nout; o++) {
		out_tracks[o] = track_alloc(tr.nbins[o % (size_t)nrec], bin);
		if (!out_tracks[o]) { tracks_drop(out_tracks, nout); return fail(E, FASIM_E_NOMEM, "out of memory"); }
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) tr.v.push_back(out_tracks[o]->v[c]);
	}
	return FASIM_OK;
}

void sites_req_init(SitesReq& sr, int32_t min_value, int32_t max_gap, bool only, int nquery, int nrec)
{
	const size_t nout = (size_t)nquery * (size_t)nrec;
	sr.min_value = min_value; sr.max_gap = max_gap; sr.only = only; sr.nrec = nrec;
	sr.runs.resize(nout); sr.sat.assign(nout, 0); sr.mu.reset(new std::mutex[(size_t)nquery]);
}

void sites_drop(fasim_sites** out_sites, size_t nout)
{
	if (out_sites) for (size_t o = 0; o < nout; o++) { fasim_sites_free(out_sites[o]); out_sites[o] = nullptr; }
}

// Intervals of one record (the kernel's runs, or the sites of shards) -> its sites: per class sorted by start, an interval that
// starts at most max_gap after the end of what has been united so far joins it (larger value, then smaller pos, then smaller enc);
// the sites by (start, cls).  Consumes `v`.
static fasim_sites* sites_build(std::vector<fasim_site>& v, int32_t min_value, int32_t max_gap)
{
	std::sort(v.begin(), v.end(), [](const fasim_site& a, const fasim_site& b) {
		if (a.cls != b.cls) return a.cls < b.cls;
		if (a.start != b.start) return a.start < b.start;
		if (a.end != b.end) return a.end < b.end;
		if (a.value != b.value) return a.value > b.value;
		if (a.pos != b.pos) return a.pos < b.pos;
		return a.enc < b.enc;
	});
	size_t n = 0;
	for (size_t i = 0; i < v.size(); i++) {
		const fasim_site x = v[i];
		if (n > 0 && v[n - 1].cls == x.cls && x.start - v[n - 1].end <= (int64_t)max_gap) {
			fasim_site& d = v[n - 1];
			d.end = std::max(d.end, x.end);
			if (x.value > d.value || (x.value == d.value && (x.pos < d.pos || (x.pos == d.pos && x.enc < d.enc)))) { d.value = x.value; d.pos = x.pos; d.enc = x.enc; }
		} else v[n++] = x;
	}
	v.resize(n);
	std::sort(v.begin(), v.end(), [](const fasim_site& a, const fasim_site& b) { return a.start != b.start ? a.start < b.start : a.cls < b.cls; });
	fasim_sites* t = (fasim_sites*)calloc(1, sizeof(fasim_sites));
	if (!t) return nullptr;
	t->s = (fasim_site*)calloc(std::max<size_t>(1, n), sizeof(fasim_site));
	if (!t->s) { free(t); return nullptr; }
	t->n = (int64_t)n; t->min_value = min_value; t->max_gap = max_gap;
	if (n) memcpy(t->s, v.data(), n * sizeof(fasim_site));
	return t;
}

int sites_req_finish(fasim_engine* E, const SitesReq& sr, fasim_sites** out_sites, const std::function<int64_t(size_t)>& units)
{
	const size_t nout = sr.runs.size();
	try {
		std::vector<fasim_site> v;
		for (size_t o = 0; o < nout; o++) {
			const std::vector<HostRun>& runs = sr.runs[o];
			v.clear(); v.reserve(runs.size());
			for (const HostRun& h : runs) { fasim_site x; x.start = h.start; x.end = h.end; x.pos = h.pos; x.value = h.value; x.enc = h.enc; x.cls = h.cls; x.reserved = 0; v.push_back(x); }
			out_sites[o] = sites_build(v, sr.min_value, sr.max_gap);
			if (!out_sites[o]) { sites_drop(out_sites, nout); return fail(E, FASIM_E_NOMEM, "out of memory"); }
			out_sites[o]->units = units(o); out_sites[o]->saturated_units = sr.sat[o]; out_sites[o]->raw_runs = (int64_t)runs.size();
		}
	} catch (const std::bad_alloc&) { sites_drop(out_sites, nout); return fail(E, FASIM_E_NOMEM, "out of memory"); }
	return FASIM_OK;
}

// fasim_scan_records_sites; `rs` hands the resolved record set to fasim_scan_records_sites_aligned (engine_site_align.cpp)
int scan_records_sites(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_result** out_results, fasim_sites** out_sites, fasim_scan_stats* totals, RecordSet& rs)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_sites) return fail(E, FASIM_E_ARG, "bad arguments");
	if (min_value < 1 || min_value > 16383) return fail(E, FASIM_E_ARG, "sites: min_value %d lies outside [1, 16383]", min_value);
	if (max_gap < 0) return fail(E, FASIM_E_ARG, "sites: max_gap %d is negative", max_gap);
	int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, true, rs);
	if (rc) return rc;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec;
	// the sites are runs of the column maxima of the systolic scan kernel: the refusals are those of the potential tracks
	rc = check_track_source(E, rna_lens, nq, pp, "sites"); if (rc) return rc;
	for (size_t o = 0; o < nout; o++) out_sites[o] = nullptr;
	if (out_results) for (size_t o = 0; o < nout; o++) out_results[o] = nullptr;
	SitesReq sr;
	sites_req_init(sr, min_value, max_gap, out_results == nullptr, nquery, nrec);
	OwnResults res(out_results, nout);
	rc = scan_records_core(E, rnas, rna_lens, nq, dna, rs.rec_off, rs.rec_len, nrec, seg_first, seg_count, pp, res.outs, totals, { &sr });
	if (rc) return rc;
	rc = sites_req_finish(E, sr, out_sites, [&](size_t o) { return res.outs[o]->stats.units; });
	if (rc && out_results) for (size_t o = 0; o < nout; o++) { fasim_result_free(out_results[o]); out_results[o] = nullptr; }
	return rc;
}

// =====================================================================================================
// C-ABI
// =====================================================================================================
extern "C" {

void fasim_params_default(fasim_params* p)
{
	p->rule = 0; p->cutLength = 5000; p->strand = 0; p->overlapLength = 100; p->ntMin = 20; p->ntMax = 100000;
	p->scoreMin = 0.0f; p->minIdentity = 60.0f; p->minStability = 1.0f; p->penaltyT = -1000; p->penaltyC = 0;
	p->cDistance = 15; p->cLength = 50; p->classicSim = 0;
}

const char* fasim_last_error(const fasim_engine* e) { return e ? e->err.c_str() : g_last_error.c_str(); }

int fasim_engine_create(int device, fasim_engine** out) { return fasim_engine_create_ex(device, 0, out); }

int fasim_engine_create_ex(int device, int32_t flags, fasim_engine** out)
{
	if (!out) return fail(nullptr, FASIM_E_ARG, "null out pointer");
	*out = nullptr;
	const bool tune = !(flags & FASIM_CREATE_NO_PROCESS_TUNING);
	// fasim_scan keeps ~10 batches in flight on as many streams; the HIP runtime multiplexes streams onto 4 hardware
	// queues unless told otherwise, which serialises unrelated batches.  Only effective before the runtime initialises
	// (a host application that touches HIP earlier should export GPU_MAX_HW_QUEUES itself).
	if (tune) setenv("GPU_MAX_HW_QUEUES", "8", 0);
	// Host allocator: every batch builds and drops tables of a few MB on its host threads.  glibc hands such blocks back to the
	// kernel (munmap / heap trimming), and while the address space of a process with live HIP queues changes, the driver's MMU
	// notifier holds those queues up (a 120 ms kernel that overlaps the freeing of half a million strings takes 190-250 ms:
	// tools/iso_probe.py).  Keeping freed blocks of up to 32 MB in the heap removes most of that: 2.42 -> 2.38 s per 50 Mb scan
	// (profiles/r02_ab_malloc.txt).  Process-wide settings; FASIM_MALLOPT=0 leaves the allocator alone.
	if (tune) {
		static const bool once = [] {
			const char* e = getenv("FASIM_MALLOPT");
			if (e && atoi(e) == 0) return false;
			(void)mallopt(M_MMAP_THRESHOLD, 32 * 1024 * 1024);
			(void)mallopt(M_TRIM_THRESHOLD, 0x7fffffff);
			(void)mallopt(M_TOP_PAD, 256 * 1024 * 1024);
			return true;
		}();
		(void)once;
	}
	int count = 0;
	hipError_t he = hipGetDeviceCount(&count);
	if (he != hipSuccess || count <= 0) return fail(nullptr, FASIM_E_NODEVICE, "no HIP device available (%s); this library has no CPU fallback", hipGetErrorString(he));
	if (device < 0 || device >= count) return fail(nullptr, FASIM_E_NODEVICE, "device %d out of range (%d devices)", device, count);
	{
		// Host threads SLEEP in hipStreamSynchronize instead of polling: with ten batches in flight ten threads otherwise spin
		// through a scan -- 12 of the 25 CPU-seconds a 50 Mb scan costs -- on cores the host side of the batches needs (an 8-GPU
		// node gives each rank a fraction of its cores).  The flag only takes effect before the device's context exists; a host
		// application that touches HIP first (PyTorch) has to set it itself (bench.py does).  An event created with
		// hipEventBlockingSync does not have this effect on ROCm 7.2.  FASIM_BLOCKING_SYNC=0 leaves the polling wait.
		const char* e = getenv("FASIM_BLOCKING_SYNC");
		if (tune && !(e && atoi(e) == 0)) { (void)hipSetDevice(device); (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync); (void)hipGetLastError(); }
	}
	fasim_engine* E = new fasim_engine();
	E->device = device;
	he = hipSetDevice(device);
	// one stream per engine (CU-masked and prioritised second streams for the two VALU-bound kernels were measured in round 2 and
	// lost: DESIGN.md section 4)
	if (he == hipSuccess) he = hipStreamCreate(&E->st);
	if (he != hipSuccess) { int rc = fail(nullptr, FASIM_E_NODEVICE, "cannot initialise device %d: %s", device, hipGetErrorString(he)); delete E; return rc; }
	E->lut1 = make_lut(true); E->lut2 = make_lut(false);
	std::vector<uint8_t> lut(48 * 256);
	build_enc_lut(lut.data());
	if (upload(E, E->enc_lut, lut.data(), lut.size()) || E->counter.ensure(64) != hipSuccess) { delete E; return FASIM_E_HIP; }
	unsigned hc = std::thread::hardware_concurrency();
	const char* env = getenv("FASIM_HOST_THREADS");
	// host side of a batch (CIGAR -> triplex record for every candidate alignment, ~1 us each): short bursts, shared by
	// the batches in flight; 3/8 of the cores (96 on the 256-thread GPU hosts) keeps the burst of a batch below ~50 ms
	E->host_threads = env ? std::max(1, atoi(env)) : (int)std::min(96u, std::max(1u, hc * 3 / 8));
	E->host_threads_total = E->host_threads;
	E->host_threads_explicit = env != nullptr;
	const char* v1 = getenv("FASIM_SCAN_V1");
	E->scan_v1 = v1 && atoi(v1) != 0;
	const char* a1 = getenv("FASIM_ALIGN_V1");
	E->align_v1 = a1 && atoi(a1) != 0;
	const char* sw = getenv("FASIM_STRIPED_WINDOW");
	E->striped_window = sw && atoi(sw) != 0;
	*out = E;
	return FASIM_OK;
}

void fasim_engine_destroy(fasim_engine* e)
{
	if (!e) return;
	for (fasim_engine* w : e->workers) fasim_engine_destroy(w);
	e->workers.clear();
	(void)hipSetDevice(e->device);
	DevBuf* bufs[] = { &e->q1, &e->q2, &e->enc_lut, &e->counter, &e->dna, &e->seg_start, &e->seg_len, &e->enc_ids, &e->tcodes,
		&e->colmax, &e->probs, &e->max_out, &e->unit_len, &e->stage1, &e->hits, &e->hits_total, &e->hit_off, &e->hit_cnt, &e->thr,
		&e->ends, &e->bprobs, &e->bout, &e->scratch, &e->dna_res, &e->colmax16, &e->unit_ids, &e->flags, &e->stage1_in, &e->hits2,
		&e->fprobs, &e->ftasks, &e->fstream, &e->fout, &e->aout, &e->cigpool, &e->cigcount, &e->forder, &e->scratch2, &e->boundary, &e->fboundary, &e->unit_hz,
		&e->unit_first, &e->hz_cols, &e->hz_plan, &e->hz_base, &e->hz_items, &e->snap, &e->hz_state, &e->hz_rows, &e->hz_chunk, &e->hz_src, &e->hz_zero,
		&e->qsim, &e->sim_min, &e->sim_row, &e->sim_ev, &e->sim_cnt, &e->sim_nodes,
		&e->ublk, &e->btarget, &e->bidx, &e->bcounts, &e->blist[0], &e->blist[1], &e->blist[2], &e->bslots[0], &e->bslots[1], &e->bslots[2],
		&e->bprev, &e->lane_ub, &e->fzones, &e->fubslot, &e->bdec, &e->btab, &e->swin, &e->unit_ovf, &e->track, &e->track_phase, &e->track_sat, &e->track_peaks, &e->sites_counts, &e->sites_offsets, &e->sites_runs, &e->sites_sat, &e->sa_q, &e->sa_tcodes, &e->sa_probs, &e->sa_ends, &e->sa_rows, &e->sa_items, &e->sa_dirs, &e->sa_cigar, &e->sa_ciglen,
		&e->rowmax16, &e->row_out, &e->row_gfirst, &e->row_sat, &e->oligo_q, &e->rowpart16, &e->hist, &e->hist_zone, &e->hist_zones, &e->hist_sat, &e->hist_pairs, &e->hist_border,
		&e->vr_q, &e->vr_dna, &e->vr_alt, &e->vr_probs, &e->vr_tcodes, &e->vr_rows, &e->vr_touch, &e->vr_out,
		&e->vr_items, &e->vr_dirs, &e->vr_cigar, &e->vr_paths, &e->vr_hwins, &e->vr_pieces, &e->vr_ends, &e->mu_first, &e->mu_groups, &e->mu_snap, &e->mu_cols, &e->mu_pm, &e->fmask, &e->flist, &e->fmarks, &e->seg_clean };
	for (auto& t : e->timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
	for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
	for (DevBuf* b : bufs) b->release();
	if (e->pin_dna) (void)hipHostFree(e->pin_dna);
	if (e->pin_sim) (void)hipHostFree(e->pin_sim);
	if (e->st) (void)hipStreamDestroy(e->st);
	delete e;
}

int fasim_set_option(fasim_engine* E, const char* key, int32_t value)
{
	if (!E || !key) return fail(E, FASIM_E_ARG, "null argument");
	if (!strcmp(key, "workers")) E->opt_workers = value > 0 ? value : 0;
	else if (!strcmp(key, "seg_batch")) E->opt_seg_batch = value > 0 ? value : 0;
	else if (!strcmp(key, "taper")) E->opt_taper = value;          // percent of the segments scanned in half-size batches at the end (-1: default)
	else if (!strcmp(key, "heavy_gate")) E->opt_gate = value;      // k_scan / k_align_fwd launches in flight at once (0: no gate, -1: default)
	else if (!strcmp(key, "hazard_chunks")) E->hz_chunks = value;          // 0: whole-unit stripe-faithful re-run; 1: column chunks (default)
	else if (!strcmp(key, "hazard_snapshots")) E->hz_snap = value;        // 0: the checkpoint pass starts every unit at column 0
	else if (!strcmp(key, "hazard_chunk_cols")) E->hz_target = value > 0 ? std::max(64, value) : 0;
	else if (!strcmp(key, "hazard_hot_weight")) E->hz_hot_w = value > 0 ? std::min(32, value) : 0;
	else if (!strcmp(key, "host_threads")) { if (value > 0) { E->host_threads = value; E->host_threads_total = value; E->host_threads_explicit = true; } }   // host side of the batches (all workers together)
	else if (!strcmp(key, "numa_affinity")) E->opt_numa = value != 0;
	else if (!strcmp(key, "band")) E->opt_band = value;                   // banded stage-3 forward pass: 0 off, 1 on (-1: default / FASIM_BAND)
	else if (!strcmp(key, "dp_f16")) E->opt_dp_f16 = value;               // 1: packed-f16 k_scan and reverse pass (default), 0: the integer kernels (-1: default / FASIM_DP_F16)
	else if (!strcmp(key, "q2_past_cut")) E->opt_q2_past_cut = value;     // 0: k_scan stops tracking Q2 taints behind a proven overflow cut (default), 1: tracks to the end of the unit (-1: default / FASIM_Q2_PAST_CUT)
	else if (!strcmp(key, "finish_skip")) E->opt_finish_skip = value;     // 1: alignments the stability filter must drop get no CIGAR (default), 0: k_finish_lds traces all, 2: trace all and check the rule (-1: default / FASIM_FINISH_SKIP)
	else if (!strcmp(key, "site_short")) E->opt_site_short = value;       // 1: the hits of oligo sites end on k_site_ends_short (default), 0: on k_site_ends (-1: default / FASIM_SITE_SHORT)
	else if (!strcmp(key, "sim_lds")) E->opt_sim_lds = value < 0 ? -1 : value != 0;   // -F re-sweeps: 0 the L2 variant, 1 the LDS variant where the state fits, -1 by the units in flight (tests)
	else if (!strcmp(key, "site_chunk")) E->opt_site_chunk = value > 0 ? value : 0;   // problems per chunk of the site hits phase (0: the phase's own limit)
	else if (!strcmp(key, "striped_window")) E->striped_window = value > 0;   // 1: every k_striped launch on the HBM-window variant (tests)
	else return fail(E, FASIM_E_ARG, "unknown option %s", key);
	return FASIM_OK;
}

int fasim_set_query(fasim_engine* E, const char* rna, int32_t len)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!rna || len <= 0) return fail(E, FASIM_E_ARG, "empty query");
	if (len > FASIM_MAX_QUERY) return refuse_long_query(E, len, -1);
	HIPOK(hipSetDevice(E->device));
	E->rna.assign(rna, rna + len);
	E->m = len;
	std::vector<uint8_t> c1(len), c2(len);
	E->query_acgt = true;
	for (int i = 0; i < len; i++) {
		c1[i] = code1(rna[i]); c2[i] = code2(rna[i]);
		const char c = rna[i];
		if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'a' || c == 'c' || c == 'g' || c == 't')) E->query_acgt = false;
	}
	std::vector<uint8_t> cs(len);
	for (int i = 0; i < len; i++) cs[i] = sim_code(rna[i]);
	int rc = upload(E, E->q1, c1.data(), len);
	if (!rc) rc = upload(E, E->q2, c2.data(), len);
	if (!rc) rc = upload(E, E->qsim, cs.data(), len);
	if (rc) return rc;
	HIPOK(hipStreamSynchronize(E->st));
	return FASIM_OK;
}

int fasim_pre_align_batch(fasim_engine* E, const char* targets, const int64_t* offsets, const int32_t* lens,
	int32_t nprob, int32_t* out_cols, int32_t* out_stage1)
{
	int rc = need_query(E); if (rc) return rc;
	if (!targets || !offsets || !lens || nprob <= 0) return fail(E, FASIM_E_ARG, "bad batch arguments");
	HIPOK(hipSetDevice(E->device));
	UnitBatch B;
	if (out_stage1) {
		rc = load_raw_targets(E, targets, offsets, lens, nprob, true, B); if (rc) return rc;
		std::vector<int> sc;
		rc = run_stage1(E, B, sc, nullptr); if (rc) return rc;
		memcpy(out_stage1, sc.data(), sizeof(int32_t) * nprob);
	}
	if (out_cols) {
		rc = load_raw_targets(E, targets, offsets, lens, nprob, false, B); if (rc) return rc;
		rc = run_stage2(E, B); if (rc) return rc;
		std::vector<uint8_t> cm((size_t)nprob * B.tstride);
		HIPOK(hipMemcpyAsync(cm.data(), E->colmax.p, cm.size(), hipMemcpyDeviceToHost, E->st));
		HIPOK(hipStreamSynchronize(E->st));
		for (int i = 0; i < nprob; i++)
			for (int c = 0; c < lens[i]; c++) out_cols[offsets[i] + c] = cm[(size_t)i * B.tstride + c];
	}
	return FASIM_OK;
}

int fasim_calc_score_once(fasim_engine* E, const char* target, int32_t n, int32_t* score)
{
	if (!target || !score) return fail(E, FASIM_E_ARG, "null argument");
	const int64_t off = 0;
	return fasim_pre_align_batch(E, target, &off, &n, 1, nullptr, score);
}

int fasim_ssw_pre_align(fasim_engine* E, const char* target, int32_t n, int32_t* out_cols)
{
	if (!target || !out_cols) return fail(E, FASIM_E_ARG, "null argument");
	const int64_t off = 0;
	return fasim_pre_align_batch(E, target, &off, &n, 1, out_cols, nullptr);
}

int fasim_ssw_colmax_word(fasim_engine* E, const char* target, int32_t n, int32_t* out_cols)
{
	int rc = need_query(E); if (rc) return rc;
	if (!target || !out_cols || n <= 0) return fail(E, FASIM_E_ARG, "bad arguments");
	HIPOK(hipSetDevice(E->device));
	UnitBatch B;
	const int64_t off = 0;
	rc = load_raw_targets(E, target, &off, &n, 1, false, B); if (rc) return rc;
	HIPOK(E->colmax16.ensure((size_t)B.tstride * sizeof(uint16_t)));
	HIPOK(E->max_out.ensure(sizeof(int32_t)));
	const std::vector<StripedProb> probs = whole_unit_probs(B, E->m, nullptr);
	rc = upload(E, E->probs, probs.data(), probs.size() * sizeof(StripedProb)); if (rc) return rc;
	StripedLaunch L;
	L.tcodes = E->tcodes.as<uint8_t>(); L.qcodes = E->q2.as<uint8_t>(); L.probs = E->probs.as<StripedProb>(); L.nprob = 1;
	L.counter = E->counter.as<uint32_t>(); L.lut = E->lut2; L.max_qlen = E->m; L.colmax = nullptr;
	L.colmax_w = E->colmax16.as<uint16_t>(); L.max_out = E->max_out.as<int32_t>(); L.ends = nullptr;
	bool win = false;
	rc = prep_striped_window(E, MODE_PRE, true, L, &win); if (rc) return rc;
	const hipError_t he = launch_striped(MODE_PRE, true, false, L, E->st);
	if (he == hipErrorInvalidValue) return fail(E, FASIM_E_UNSUPPORTED, "query of %d nt does not fit the LDS-resident striped kernel", E->m);
	if (he != hipSuccess) return fail(E, FASIM_E_HIP, "striped kernel launch failed: %s", hipGetErrorString(he));
	std::vector<uint16_t> cm((size_t)n);
	HIPOK(hipMemcpyAsync(cm.data(), E->colmax16.p, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost, E->st));
	HIPOK(hipStreamSynchronize(E->st));
	for (int c = 0; c < n; c++) out_cols[c] = cm[(size_t)c];
	return FASIM_OK;
}

int fasim_sim_finish_unit(const char* rna, int32_t m, const char* seg, int32_t n, int32_t enc, int64_t dna_start, int64_t min_score,
	const fasim_params* p, const fasim_sim_node* nodes, int32_t nnodes, fasim_result** out)
{
	if (!rna || m <= 0 || !seg || n <= 0 || enc < 0 || enc >= 48 || !p || (nnodes > 0 && !nodes) || nnodes < 0 || nnodes > FASIM_SIM_K || !out)
		return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string target, src;
	encode_unit_host(seg, n, enc, target, src);
	std::vector<fasim_sim_node> list(nodes, nodes + nnodes);
	std::vector<HostTriplex> recs;
	sim_finish_unit(std::string(rna, rna + m), target, src, (long)dna_start, (long)min_score, enc, *p, list, recs);
	for (HostTriplex& t : recs) t.enc = enc;
	fasim_scan_stats st; memset(&st, 0, sizeof st);
	return pack_result(nullptr, recs, st, out);
}

int fasim_sim_forward_batch(fasim_engine* E, const char* targets, const int64_t* offsets, const int32_t* lens, int32_t nprob,
	const int64_t* min_scores, fasim_sim_node* nodes, int32_t* counts)
{
	int rc = need_query(E); if (rc) return rc;
	if (!targets || !offsets || !lens || !min_scores || !nodes || !counts || nprob <= 0) return fail(E, FASIM_E_ARG, "bad arguments");
	HIPOK(hipSetDevice(E->device));
	int maxlen = 1;
	for (int k = 0; k < nprob; k++) {
		if (lens[k] <= 0) return fail(E, FASIM_E_ARG, "empty target %d", k);
		maxlen = std::max(maxlen, lens[k]);
	}
	const int tstride = (maxlen + 15) & ~15;
	std::vector<uint8_t> tc((size_t)nprob * tstride, 4);
	for (int k = 0; k < nprob; k++) for (int c = 0; c < lens[k]; c++) tc[(size_t)k * tstride + c] = sim_code(targets[offsets[k] + c]);
	rc = upload(E, E->tcodes, tc.data(), tc.size()); if (rc) return rc;
	rc = upload(E, E->unit_len, lens, sizeof(int32_t) * nprob); if (rc) return rc;
	std::vector<std::vector<fasim_sim_node>> lists((size_t)nprob);
	rc = sim_forward_units(E, E->tcodes.as<uint8_t>(), tstride, E->unit_len.as<int32_t>(), lens, 0, nprob, min_scores, nullptr, lists);
	if (rc) return rc;
	for (int k = 0; k < nprob; k++) {
		counts[k] = (int32_t)lists[(size_t)k].size();
		for (size_t x = 0; x < lists[(size_t)k].size(); x++) nodes[(size_t)k * FASIM_SIM_K + x] = lists[(size_t)k][x];
	}
	drain_timed(E);
	return FASIM_OK;
}

int fasim_selfcheck_records(uint64_t seed, int32_t n, int32_t* mismatches)
{
	if (!mismatches || n <= 0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	uint64_t x = seed ? seed : 1;
	auto rnd = [&]() { x += 0x9E3779B97F4A7C15ull; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
	const char letters[] = "ACGTACGTACGTNacgt";
	std::string seg(5000, 'A'), rna(3000, 'A');
	for (char& c : seg) c = letters[rnd() % (sizeof letters - 1)];
	for (char& c : rna) c = "ACGU"[rnd() % 4];
	fasim_params p; fasim_params_default(&p);
	int bad = 0;
	const bool acgtn = false;
	std::vector<HostTriplex> hs; std::vector<TriplexNum> ns;
	for (int k = 0; k < n; k++) {
		// a random alignment: a few runs of M / I / D inside the segment and the lncRNA
		AlignResult al; memset(&al, 0, sizeof al);
		uint32_t cig[16]; int nc = 1 + (int)(rnd() % 6), ref = 0, qry = 0;
		for (int c = 0; c < nc; c++) { const uint32_t op = c % 2 == 0 ? 0u : 1u + (uint32_t)(rnd() % 2), len = 1 + (uint32_t)(rnd() % (op == 0 ? 40 : 3)); cig[c] = (len << 4) | op; if (op != 1) ref += (int)len; if (op != 2) qry += (int)len; }
		al.cigar_off = 0; al.cigar_len = nc; al.sw_score = 20 + (int)(rnd() % 200);
		al.ref_begin = (int)(rnd() % (uint64_t)(5000 - ref)); al.ref_end = al.ref_begin + ref - 1;
		al.query_begin = (int)(rnd() % (uint64_t)(3000 - qry)); al.query_end = al.query_begin + qry - 1;
		const int enc = (int)(rnd() % 48);
		std::vector<HostTriplex> a, b; std::vector<TriplexNum> c;
		convert_triplex(al, cig, rna, seg.data(), 5000, enc, 1000, p, a, acgtn, true);
		convert_triplex(al, cig, rna, seg.data(), 5000, enc, 1000, p, b, acgtn, false);
		convert_triplex_num(al, cig, rna, seg.data(), 5000, enc, 1000, p, c, acgtn);
		if (a.size() != b.size() || a.size() != c.size()) { bad++; continue; }
		if (a.empty()) continue;
		const HostTriplex& s1 = a[0]; const HostTriplex& s2 = b[0]; const TriplexNum& s3 = c[0];
		auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
		if (s1.stari != s3.stari || s1.endi != s3.endi || s1.starj != s3.starj || s1.endj != s3.endj || s1.nt != s3.nt || bits(s1.score) != bits(s3.score) ||
			bits(s1.identity) != bits(s3.identity) || bits(s1.tri_score) != bits(s3.tri_score) || bits(s2.identity) != bits(s1.identity) || bits(s2.tri_score) != bits(s1.tri_score)) bad++;
		// the same record, squeezed into a small coordinate range so that the dedup sees ties, containments and equal scores
		HostTriplex h = s2; h.stari = 1 + (int)(rnd() % 6); h.endi = h.stari + (int)(rnd() % 6); h.starj = 100 + (int)(rnd() % 6); h.endj = h.starj + (int)(rnd() % 6);
		h.score = (float)(50 + rnd() % 4); h.cand = k;
		TriplexNum t; t.stari = h.stari; t.endi = h.endi; t.starj = h.starj; t.endj = h.endj; t.nt = h.nt; t.cand = k; t.score = h.score; t.identity = h.identity; t.tri_score = h.tri_score;
		hs.push_back(h); ns.push_back(t);
		if (hs.size() == 40 || k == n - 1) {
			std::vector<HostTriplex> oh; std::vector<TriplexNum> on;
			dedup_top(hs, p, oh); dedup_top_num(ns, p, on);
			if (oh.size() != on.size()) bad++;
			else for (size_t i = 0; i < oh.size(); i++) if (oh[i].cand != on[i].cand) bad++;
			hs.clear(); ns.clear();
		}
	}
	*mismatches = bad;
	return FASIM_OK;
}

int fasim_pick_candidates(const int32_t* cols, int32_t n, int32_t threshold, int32_t* out_score, int32_t* out_pos,
	int32_t cap, int32_t* count)
{
	if (!cols || !count || n < 0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::vector<uint32_t> hits;
	for (int c = 0; c < n; c++) if (cols[c] > threshold) hits.push_back(((uint32_t)c << 8) | (uint32_t)(cols[c] & 0xff));
	std::vector<Cand> cands;
	pick_candidates(hits.data(), (int)hits.size(), cands);
	*count = (int)cands.size();
	for (int i = 0; i < (int)cands.size() && i < cap; i++) { if (out_score) out_score[i] = cands[i].score; if (out_pos) out_pos[i] = cands[i].pos; }
	return FASIM_OK;
}

int fasim_align_batch(fasim_engine* E, const char* windows, const int64_t* offsets, const int32_t* lens, int32_t nprob,
	fasim_alignment* out)
{
	return fasim_align_batch_ex(E, windows, offsets, lens, nprob, out, nullptr);
}

int fasim_align_batch_ex(fasim_engine* E, const char* windows, const int64_t* offsets, const int32_t* lens, int32_t nprob,
	fasim_alignment* out, int32_t* path)
{
	int rc = need_query(E); if (rc) return rc;
	if (!windows || !offsets || !lens || !out || nprob <= 0) return fail(E, FASIM_E_ARG, "bad batch arguments");
	HIPOK(hipSetDevice(E->device));
	UnitBatch B;
	rc = load_raw_targets(E, windows, offsets, lens, nprob, false, B); if (rc) return rc;
	std::vector<WindowProb> W(nprob);
	for (int i = 0; i < nprob; i++) { W[i].unit = i; W[i].t0 = 0; W[i].len = lens[i]; }
	std::vector<AlignResult> res;
	std::vector<uint32_t> cigars;
	std::vector<int32_t> how;
	rc = run_align_v2(E, B, W, res, cigars, nullptr, path ? &how : nullptr); if (rc) return rc;
	if (path) memcpy(path, how.data(), sizeof(int32_t) * (size_t)nprob);
	for (int i = 0; i < nprob; i++) {
		out[i].sw_score = res[i].sw_score; out[i].ref_begin = res[i].ref_begin; out[i].ref_end = res[i].ref_end;
		out[i].query_begin = res[i].query_begin; out[i].query_end = res[i].query_end;
		// (the finish kernels hold at most ALIGN_MAX_CIGAR = 48 runs and hand longer CIGARs to the replay, whose traceback holds
		//  MAX_CIGAR_DEV = 62 and fails loudly beyond that; never hand back a truncated CIGAR)
		if (res[i].cigar_len > 256) return fail(E, FASIM_E_UNSUPPORTED, "alignment %d has %d CIGAR runs; fasim_alignment holds 256", i, res[i].cigar_len);
		out[i].cigar_len = res[i].cigar_len;
		if (out[i].cigar_len) memcpy(out[i].cigar, cigars.data() + res[i].cigar_off, sizeof(uint32_t) * out[i].cigar_len);
		if (res[i].failed) { out[i].sw_score = 0; out[i].cigar_len = -1; }     // the reference returns NULL here
	}
	return FASIM_OK;
}

int fasim_ssw_align(fasim_engine* E, const char* window, int32_t n, fasim_alignment* out)
{
	const int64_t off = 0;
	return fasim_align_batch(E, window, &off, &n, 1, out);
}

int fasim_encode_unit(const char* seg, int32_t n, int32_t enc, char* target, char* src)
{
	if (!seg || n < 0 || enc < 0 || enc >= 48 || !target || !src) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string t, s;
	encode_unit_host(seg, n, enc, t, s);
	memcpy(target, t.data(), n);
	memset(src, 0, n);
	memcpy(src, s.data(), s.size());
	return FASIM_OK;
}

int fasim_load_dna(fasim_engine* E, const char* dna, int64_t dna_len)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!dna || dna_len <= 0) return fail(E, FASIM_E_ARG, "empty DNA");
	// (a resident record set may be longer than 2^31 nt: fasim_scan refuses a single record above it, fasim_scan_records a record)
	HIPOK(hipSetDevice(E->device));
	E->dna_host.assign(dna, dna + dna_len);
	int rc = upload(E, E->dna_res, dna, (size_t)dna_len);
	if (rc) { E->dna_host.clear(); return rc; }
	return FASIM_OK;
}

int64_t fasim_segment_count(int64_t dna_len, const fasim_params* p) { return segment_count(dna_len, p); }

void fasim_result_free(fasim_result* r)
{
	if (!r) return;
	free(r->recs); free(r->pool); free(r);
}

void fasim_free(void* p) { free(p); }

int fasim_maximum3_f16(fasim_engine* E, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out3, uint32_t* out0, int64_t n)
{
	if (!E || !a || !b || !c || !out3 || !out0 || n <= 0 || n > (1ll << 28)) return fail(E, FASIM_E_ARG, "bad arguments");
	HIPOK(hipSetDevice(E->device));
	const size_t bytes = sizeof(uint32_t) * (size_t)n;
	DevBuf d[5];
	int rc = FASIM_OK;
	for (int k = 0; k < 5 && !rc; k++) if (d[k].ensure(bytes) != hipSuccess) rc = fail(E, FASIM_E_HIP, "out of device memory");
	const uint32_t* src[3] = { a, b, c };
	for (int k = 0; k < 3 && !rc; k++) if (hipMemcpyAsync(d[k].p, src[k], bytes, hipMemcpyHostToDevice, E->st) != hipSuccess) rc = fail(E, FASIM_E_HIP, "copy failed");
	if (!rc && launch_maximum3_f16(d[0].as<uint32_t>(), d[1].as<uint32_t>(), d[2].as<uint32_t>(), d[3].as<uint32_t>(), d[4].as<uint32_t>(), n, E->st) != hipSuccess)
		rc = fail(E, FASIM_E_HIP, "maximum3 launch failed");
	if (!rc && (hipMemcpyAsync(out3, d[3].p, bytes, hipMemcpyDeviceToHost, E->st) != hipSuccess ||
	            hipMemcpyAsync(out0, d[4].p, bytes, hipMemcpyDeviceToHost, E->st) != hipSuccess ||
	            hipStreamSynchronize(E->st) != hipSuccess)) rc = fail(E, FASIM_E_HIP, "copy back failed");
	(void)hipStreamSynchronize(E->st);
	for (DevBuf& x : d) x.release();
	return rc;
}

void fasim_synth_dna(char* out, int64_t n, uint64_t seed)
{
	// splitmix64, 2 bits per base, 32 bases per word (tools/synth.py random_dna)
	uint64_t s = seed;
	for (int64_t i = 0; i < n; i += 32) {
		s += 0x9E3779B97F4A7C15ull;
		uint64_t z = s;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z ^= z >> 31;
		for (int k = 0; k < 32 && i + k < n; k++) out[i + k] = "ACGT"[(z >> (2 * k)) & 3];
	}
}

int fasim_scan(fasim_engine* E, const char* dna, int64_t dna_len, int64_t seg_first, int64_t seg_count,
	const fasim_params* pp, fasim_result** out)
{
	int rc = need_query(E); if (rc) return rc;
	if (!out) return fail(E, FASIM_E_ARG, "bad arguments");
	return scan_core(E, nullptr, nullptr, 0, dna, dna_len, seg_first, seg_count, pp, out);
}

int fasim_scan_queries(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	int64_t dna_len, int64_t seg_first, int64_t seg_count, const fasim_params* pp, fasim_result** outs)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (nq <= 0 || !rnas || !rna_lens || !outs) return fail(E, FASIM_E_ARG, "bad arguments");
	for (int32_t q = 0; q < nq; q++) if (rna_lens[q] > FASIM_MAX_QUERY) return refuse_long_query(E, rna_lens[q], q);
	return scan_core(E, rnas, rna_lens, nq, dna, dna_len, seg_first, seg_count, pp, outs);
}

int fasim_scan_records(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_result** outs, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!outs) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	const int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, false, rs);
	if (rc) return rc;
	return scan_records_core(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, outs, totals);
}

// ---- per-base potential tracks ----------------------------------------------------------------------------------------
void fasim_track_free(fasim_track* t)
{
	if (!t) return;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) free(t->v[c]);
	free(t);
}

int fasim_scan_track(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna, int64_t dna_len,
	int64_t seg_first, int64_t seg_count, const fasim_params* pp, int32_t bin, fasim_result** out_results, fasim_track** out_tracks)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_tracks || !pp || nq < 0) return fail(E, FASIM_E_ARG, "bad arguments");
	if (bin < 1) return fail(E, FASIM_E_ARG, "track bin width %d: must be at least 1", bin);
	const int nquery = std::max(1, nq);
	for (int q = 0; q < nquery; q++) out_tracks[q] = nullptr;
	if (out_results) for (int q = 0; q < nquery; q++) out_results[q] = nullptr;
	if (nq == 0) { int rc = need_query(E); if (rc) return rc; }
	else {
		if (!rnas || !rna_lens) return fail(E, FASIM_E_ARG, "bad arguments");
		for (int32_t q = 0; q < nq; q++) {
			if (!rnas[q] || rna_lens[q] <= 0) return fail(E, FASIM_E_ARG, "empty query %d", q);
			if (rna_lens[q] > FASIM_MAX_QUERY) return refuse_long_query(E, rna_lens[q], q);
		}
	}
	{ const int rc = check_track_source(E, rna_lens, nq, pp); if (rc) return rc; }
	if (dna == nullptr) {
		if (E->dna_host.empty()) return fail(E, FASIM_E_ARG, "no resident DNA: call fasim_load_dna first");
		dna_len = (int64_t)E->dna_host.size();
	} else if (dna_len <= 0) return fail(E, FASIM_E_ARG, "bad arguments");
	if (dna_len > 0x7fffffffll) return fail(E, FASIM_E_ARG, "one record is limited to 2^31-1 nt (the reference's int positions)");
	TrackReq tr;
	int rc = track_req_init(E, tr, bin, out_results == nullptr, nquery, &dna_len, 1, out_tracks, nullptr); if (rc) return rc;
	OwnResults res(out_results, (size_t)nquery);
	rc = scan_core(E, nq ? rnas : nullptr, nq ? rna_lens : nullptr, nq, dna, dna_len, seg_first, seg_count, pp, res.outs, { &tr });
	if (rc) { tracks_drop(out_tracks, (size_t)nquery); return rc; }
	for (int q = 0; q < nquery; q++) { out_tracks[q]->units = res.outs[q]->stats.units; out_tracks[q]->saturated_units = tr.sat[(size_t)q]; }
	return FASIM_OK;
}

// ---- record sets screened by potential ---------------------------------------------------------
int fasim_scan_records_track(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp, int32_t bin,
	fasim_result** out_results, fasim_track** out_tracks, fasim_peak* out_peaks, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (bin < 0) return fail(E, FASIM_E_ARG, "track bin width %d: must be at least 1, or 0 for peaks only", bin);
	if (bin == 0 && (out_tracks || !out_peaks)) return fail(E, FASIM_E_ARG, "bin 0 is peaks only: out_tracks must be NULL and out_peaks must not");
	if (bin >= 1 && !out_tracks) return fail(E, FASIM_E_ARG, "bin %d needs out_tracks", bin);
	RecordSet rs;
	int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, false, rs);
	if (rc) return rc;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec;
	rc = check_track_source(E, rna_lens, nq, pp); if (rc) return rc;
	if (out_tracks) for (size_t o = 0; o < nout; o++) out_tracks[o] = nullptr;
	if (out_results) for (size_t o = 0; o < nout; o++) out_results[o] = nullptr;
	TrackReq tr;
	rc = track_req_init(E, tr, bin, out_results == nullptr, nquery, rec_len, nrec, out_tracks, out_peaks); if (rc) return rc;
	OwnResults res(out_results, nout);
	rc = scan_records_core(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, res.outs, totals, { &tr });
	if (rc) { tracks_drop(out_tracks, nout); return rc; }
	if (out_tracks) for (size_t o = 0; o < nout; o++) { out_tracks[o]->units = res.outs[o]->stats.units; out_tracks[o]->saturated_units = tr.sat[o]; }
	return FASIM_OK;
}

// ---- per-base profile of the lncRNA ------------------------------------------------------------
void fasim_tfo_profile_free(fasim_tfo_profile* t)
{
	if (!t) return;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) free(t->v[c]);
	free(t);
}

int fasim_scan_tfo_profile(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp, int32_t per_record,
	fasim_result** out_results, fasim_tfo_profile** out_profiles, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_profiles) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, false, rs);
	if (rc) return rc;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec, nprof = per_record ? nout : (size_t)nquery;
	// the profile is the row maxima of the systolic scan kernel: the refusals are those of the potential tracks
	rc = check_track_source(E, rna_lens, nq, pp); if (rc) return rc;
	for (size_t o = 0; o < nprof; o++) out_profiles[o] = nullptr;
	if (out_results) for (size_t o = 0; o < nout; o++) out_results[o] = nullptr;
	TfoReq pr;
	pr.only = out_results == nullptr; pr.per_record = per_record != 0; pr.nrec = nrec;
	pr.units.assign(nprof, 0); pr.sat.assign(nprof, 0); pr.mu.reset(new std::mutex[(size_t)nquery]);
	for (int q = 0; q < nquery; q++) pr.m.push_back(nq == 0 ? E->m : rna_lens[q]);
	auto drop = [&]() { for (size_t o = 0; o < nprof; o++) { fasim_tfo_profile_free(out_profiles[o]); out_profiles[o] = nullptr; } };
	pr.v.reserve(nprof * 4);
	for (size_t o = 0; o < nprof; o++) {
		out_profiles[o] = tfo_profile_alloc(pr.m[per_record ? o / (size_t)nrec : o]);
		if (!out_profiles[o]) { drop(); return fail(E, FASIM_E_NOMEM, "out of memory"); }
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) pr.v.push_back(out_profiles[o]->v[c]);
	}
	OwnResults res(out_results, nout);
	rc = scan_records_core(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, res.outs, totals, { &pr });
	if (rc) { drop(); return rc; }
	for (size_t o = 0; o < nprof; o++) { out_profiles[o]->units = pr.units[o]; out_profiles[o]->saturated_units = pr.sat[o]; }
	return FASIM_OK;
}

int fasim_tfo_profile_merge(const fasim_tfo_profile* const* parts, int32_t nparts, fasim_tfo_profile** out)
{
	if (!parts || nparts < 1 || !out) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr;
	for (int k = 0; k < nparts; k++) {
		if (!parts[k] || parts[k]->m < 0) return fail(nullptr, FASIM_E_ARG, "bad profile %d", k);
		if (parts[k]->m != parts[0]->m)
			return fail(nullptr, FASIM_E_ARG, "profile %d has %d bases, profile 0 has %d: only profiles of one lncRNA merge", k, parts[k]->m, parts[0]->m);
	}
	fasim_tfo_profile* t = tfo_profile_alloc(parts[0]->m);
	if (!t) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	for (int k = 0; k < nparts; k++) {
		t->units += parts[k]->units; t->saturated_units += parts[k]->saturated_units;
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			const uint16_t* src = parts[k]->v[c]; uint16_t* dst = t->v[c];
			for (int32_t i = 0; i < t->m; i++) dst[i] = std::max(dst[i], src[i]);
		}
	}
	*out = t;
	return FASIM_OK;
}

int fasim_tfo_profile_tsv(const fasim_tfo_profile* t, const char* rna, const char* rna_name, char** text, int64_t* text_len)
{
	if (!t || !rna || !text || !text_len || t->m < 0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	(void)rna_name;      // (the table itself carries no name: the caller names the file)
	std::string o = "pos\tbase\tParaPlus\tParaMinus\tAntiMinus\tAntiPlus\n";
	char line[96];
	for (int32_t i = 0; i < t->m; i++) {
		const int n = snprintf(line, sizeof line, "%d\t%c\t%d\t%d\t%d\t%d\n", i + 1, rna[i], (int)t->v[0][i], (int)t->v[1][i], (int)t->v[2][i], (int)t->v[3][i]);
		o.append(line, (size_t)n);
	}
	return text_out(o, text, text_len);
}

int fasim_peaks_merge(const fasim_peak* const* parts, int32_t nparts, int64_t n, fasim_peak* out)
{
	if (!parts || nparts < 1 || n < 0 || (n > 0 && !out)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	for (int k = 0; k < nparts; k++) if (!parts[k] && n > 0) return fail(nullptr, FASIM_E_ARG, "bad part %d", k);
	for (int64_t i = 0; i < n; i++) {
		fasim_peak d = parts[0][i];
		for (int k = 1; k < nparts; k++) {
			const fasim_peak& x = parts[k][i];
			if (x.value > d.value || (x.value == d.value && (x.pos < d.pos || (x.pos == d.pos && x.enc < d.enc)))) d = x;
		}
		out[i] = d;
	}
	return FASIM_OK;
}

int fasim_screen_tsv(const fasim_region* regions, const int64_t* segments, const fasim_peak* peaks, int64_t n, char** text, int64_t* text_len)
{
	if (n < 0 || !text || !text_len || (n > 0 && (!regions || !segments || !peaks))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::string o = "line\tname\tchrom\tstart\tend\tsegments";
	for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "\t"; o += c; o += "_pos\t"; o += c; o += "_rule"; }
	o += "\n";
	for (int64_t k = 0; k < n; k++) {
		const fasim_region& g = regions[k];
		if (!g.name || !g.chrom) return fail(nullptr, FASIM_E_ARG, "interval %lld has no name or chromosome", (long long)k);
		o += std::to_string(g.line); o += "\t"; o += g.name; o += "\t"; o += g.chrom; o += "\t"; o += std::to_string(g.start); o += "\t"; o += std::to_string(g.end);
		if (segments[k] < 0) { for (int c = 0; c < 1 + 3 * FASIM_TRACK_CLASSES; c++) o += "\tNA"; o += "\n"; continue; }
		o += "\t"; o += std::to_string(segments[k]);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			const fasim_peak& pk = peaks[k * FASIM_TRACK_CLASSES + c];
			if (pk.value <= 0 || pk.enc < 0 || pk.enc >= 48) { o += "\t0\tNA\tNA"; continue; }
			o += "\t"; o += std::to_string(pk.value); o += "\t"; o += std::to_string(g.start + pk.pos); o += "\t"; o += std::to_string(enc_info(pk.enc).rule);
		}
		o += "\n";
	}
	return text_out(o, text, text_len);
}

int fasim_track_merge(const fasim_track* const* parts, int32_t nparts, fasim_track** out)
{
	if (!parts || nparts < 1 || !out) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr;
	for (int k = 0; k < nparts; k++) {
		if (!parts[k] || parts[k]->bin < 1 || parts[k]->nbins < 0) return fail(nullptr, FASIM_E_ARG, "bad track %d", k);
		if (parts[k]->bin != parts[0]->bin || parts[k]->nbins != parts[0]->nbins)
			return fail(nullptr, FASIM_E_ARG, "track %d has bin %d and %lld bins, track 0 has bin %d and %lld bins: only tracks of one record and one bin width merge",
				k, parts[k]->bin, (long long)parts[k]->nbins, parts[0]->bin, (long long)parts[0]->nbins);
	}
	fasim_track* t = track_alloc(parts[0]->nbins, parts[0]->bin);
	if (!t) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	for (int k = 0; k < nparts; k++) {
		t->units += parts[k]->units; t->saturated_units += parts[k]->saturated_units;
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
			const uint16_t* src = parts[k]->v[c]; uint16_t* dst = t->v[c];
			for (int64_t i = 0; i < t->nbins; i++) dst[i] = std::max(dst[i], src[i]);
		}
	}
	*out = t;
	return FASIM_OK;
}

int fasim_track_bedgraph(const fasim_track* t, const char* chr, int64_t start_genome, int64_t dna_len, const char* rna_name,
	int32_t min_value, char** text, int64_t* text_len)
{
	if (!t || !chr || !rna_name || !text || !text_len || t->bin < 1) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (min_value < 1) return fail(nullptr, FASIM_E_ARG, "min_value %d: must be at least 1 (bins of value 0 are never written)", min_value);
	if (dna_len <= 0 || (dna_len + t->bin - 1) / t->bin != t->nbins) return fail(nullptr, FASIM_E_ARG, "dna_len %lld does not match a track of %lld bins of %d", (long long)dna_len, (long long)t->nbins, t->bin);
	const int64_t sg = start_genome - 1;                  // 0-based genome position of the record's first base
	std::string o;
	char line[96];
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
		o += "track type=bedGraph name='"; o += rna_name; o += " potential ("; o += CLASS_NAMES[c]; o += ")'\n";
		const uint16_t* v = t->v[c];
		for (int64_t b = 0; b < t->nbins; ) {
			int64_t e = b + 1;
			while (e < t->nbins && v[e] == v[b]) e++;
			if (v[b] >= min_value) {
				const int n = snprintf(line, sizeof line, "\t%lld\t%lld\t%d\n", (long long)(sg + b * t->bin), (long long)(sg + std::min<int64_t>(e * t->bin, dna_len)), (int)v[b]);
				o += chr; o.append(line, (size_t)n);
			}
			b = e;
		}
	}
	return text_out(o, text, text_len);
}

// ---- sites above a fixed potential -------------------------------------------------------------
void fasim_sites_free(fasim_sites* t)
{
	if (!t) return;
	free(t->s);
	free(t);
}

int fasim_scan_records_sites(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_result** out_results, fasim_sites** out_sites, fasim_scan_stats* totals)
{
	RecordSet rs;
	return scan_records_sites(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, min_value, max_gap, out_results, out_sites, totals, rs);
}

int fasim_sites_merge(const fasim_sites* const* parts, int32_t nparts, fasim_sites** out)
{
	if (!parts || nparts < 1 || !out) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr;
	size_t total = 0;
	for (int k = 0; k < nparts; k++) {
		if (!parts[k] || parts[k]->n < 0 || (parts[k]->n > 0 && !parts[k]->s)) return fail(nullptr, FASIM_E_ARG, "bad site list %d", k);
		if (parts[k]->min_value != parts[0]->min_value || parts[k]->max_gap != parts[0]->max_gap)
			return fail(nullptr, FASIM_E_ARG, "site list %d has min_value %d and max_gap %d, list 0 has %d and %d: only lists of one threshold and gap merge",
				k, parts[k]->min_value, parts[k]->max_gap, parts[0]->min_value, parts[0]->max_gap);
		total += (size_t)parts[k]->n;
	}
	fasim_sites* t = nullptr;
	try {
		std::vector<fasim_site> v;
		v.reserve(total);
		for (int k = 0; k < nparts; k++) v.insert(v.end(), parts[k]->s, parts[k]->s + parts[k]->n);
		for (fasim_site& x : v) x.reserved = 0;
		t = sites_build(v, parts[0]->min_value, parts[0]->max_gap);
	} catch (const std::bad_alloc&) { t = nullptr; }
	if (!t) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	for (int k = 0; k < nparts; k++) { t->units += parts[k]->units; t->saturated_units += parts[k]->saturated_units; t->raw_runs += parts[k]->raw_runs; }
	*out = t;
	return FASIM_OK;
}

int fasim_sites_bed(const fasim_sites* t, const char* chr, int64_t start_genome, const char* rna_name, const char* record_name,
	int32_t header, char** text, int64_t* text_len)
{
	if (!t || !chr || !rna_name || !text || !text_len || t->n < 0 || (t->n > 0 && !t->s)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	const int64_t sg = start_genome - 1;                  // 0-based genome position of the record's first base
	std::string o;
	char line[160];
	if (header) { o += "# fasim sites lncRNA="; o += rna_name; o += " min_value="; o += std::to_string(t->min_value); o += " max_gap="; o += std::to_string(t->max_gap); o += "\n"; }
	for (int64_t i = 0; i < t->n; i++) {
		const fasim_site& x = t->s[i];
		if (x.cls < 0 || x.cls >= FASIM_TRACK_CLASSES || x.enc < 0 || x.enc >= 48) return fail(nullptr, FASIM_E_ARG, "site %lld has class %d and encoding %d", (long long)i, x.cls, x.enc);
		const int n = snprintf(line, sizeof line, "\t%lld\t%lld\t%s\t%d\t%c\t%lld\t%d", (long long)(sg + x.start), (long long)(sg + x.end), CLASS_NAMES[x.cls], x.value,
			(x.cls == 0 || x.cls == 3) ? '+' : '-', (long long)(sg + x.pos), enc_info(x.enc).rule);
		o += chr; o.append(line, (size_t)n);
		if (record_name) { o += "\t"; o += record_name; }
		o += "\n";
	}
	return text_out(o, text, text_len);
}

// in-place variant for a gather that already placed every shard's records and pool at their final positions
int fasim_rebase_offsets(fasim_triplex* recs, int64_t count, int64_t delta)
{
	if (count < 0 || (count > 0 && !recs)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	for (int64_t i = 0; i < count; i++) { recs[i].tfo_off += delta; recs[i].tts_off += delta; }
	return FASIM_OK;
}

// ---- the exchange step's host half: shard results -> one result, in the order given ------------------------------
int fasim_merge_results(const fasim_triplex* const* recs, const int64_t* counts, const char* const* pools,
	const int64_t* pool_lens, int32_t nparts, fasim_result** out)
{
	if (nparts < 0 || !out || (nparts > 0 && (!recs || !counts || !pools || !pool_lens))) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	int64_t total = 0, pool_total = 0;
	std::vector<int64_t> rbase((size_t)nparts), pbase((size_t)nparts);
	for (int k = 0; k < nparts; k++) {
		if (counts[k] < 0 || pool_lens[k] < 0 || (counts[k] > 0 && (!recs[k] || !pools[k]))) return fail(nullptr, FASIM_E_ARG, "bad part %d", k);
		rbase[(size_t)k] = total; pbase[(size_t)k] = pool_total;
		total += counts[k]; pool_total += pool_lens[k];
	}
	fasim_result* R = (fasim_result*)calloc(1, sizeof(fasim_result));
	if (!R) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	R->recs = (fasim_triplex*)malloc(std::max<size_t>(1, (size_t)total) * sizeof(fasim_triplex));
	R->pool = (char*)malloc(std::max<size_t>(1, (size_t)pool_total));
	if (!R->recs || !R->pool) { fasim_result_free(R); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	R->count = total; R->pool_len = pool_total;
	// one pass per part: copy the records with their pool offsets rebased, copy the pool; parts are independent, so
	// large merges run one host thread per part
	auto one = [&](int k) {
		fasim_triplex* dst = R->recs + rbase[(size_t)k];
		const fasim_triplex* src = recs[k];
		const int64_t pb = pbase[(size_t)k];
		for (int64_t i = 0; i < counts[k]; i++) { fasim_triplex t = src[i]; t.tfo_off += pb; t.tts_off += pb; dst[i] = t; }
		if (pool_lens[k]) memcpy(R->pool + pb, pools[k], (size_t)pool_lens[k]);
	};
	if (nparts > 1 && total + pool_total / 64 > 100000) {
		std::vector<std::thread> th;
		for (int k = 0; k < nparts; k++) th.emplace_back(one, k);
		for (auto& t : th) t.join();
	} else for (int k = 0; k < nparts; k++) one(k);
	*out = R;
	return FASIM_OK;
}

static int records_to_list(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len, const fasim_params* p,
	int64_t start_genome, int32_t flags, std::vector<HostTriplex>& list)
{
	list.resize((size_t)count);
	for (int64_t i = 0; i < count; i++) {
		const fasim_triplex& r = recs[i];
		if (pool && (r.tfo_off < 0 || r.tfo_off >= pool_len || r.tts_off < 0 || r.tts_off >= pool_len)) return fail(nullptr, FASIM_E_ARG, "record %lld points outside the pool", (long long)i);
		HostTriplex& t = list[(size_t)i];
		t.stari = r.stari; t.endi = r.endi; t.starj = r.starj; t.endj = r.endj; t.strand = r.strand; t.reverse = r.reverse;
		t.rule = r.rule; t.nt = r.nt; t.score = r.score; t.identity = r.identity; t.tri_score = r.tri_score; t.seg = r.seg; t.enc = r.enc;
		t.tfo = pool ? pool + r.tfo_off : ""; t.tts = pool ? pool + r.tts_off : "";
		// records of a later FASTA record in the reference's accumulating reader carry their own genome start (main(),
		// Fasim-LongTarget.cpp:141-149 patches each record's triplexes with startGenomeTmp[i])
		if (r.genome_shift != 0) { t.genomestart = (long)r.starj + (long)start_genome + r.genome_shift - 1; t.genomeend = (long)r.endj + (long)start_genome + r.genome_shift - 1; t.genome_set = true; }
		if (t.nt > p->cLength && (t.stari + t.endi) / 2 - p->cDistance < 0 && !(flags & FASIM_TAIL_CLAMP_CLUSTER))
			return fail(nullptr, FASIM_E_UNSUPPORTED, "a triplex mid-point lies within -ds of the query start: the reference's clustering does not terminate for this input (FASIM_TAIL_CLAMP_CLUSTER / fasim --clamp-cluster gives a defined result)");
	}
	return FASIM_OK;
}

int fasim_tfosorted_ex(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len, const char* chr,
	int64_t start_genome, const fasim_params* p, int32_t flags, char** text, int64_t* text_len)
{
	if ((count > 0 && (!recs || !pool)) || !chr || !p || !text || !text_len || count < 0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::vector<HostTriplex> list;
	const int rc = records_to_list(recs, count, pool, pool_len, p, start_genome, flags, list);
	if (rc != FASIM_OK) return rc;
	return text_out(tfosorted_text(list, chr, (long)start_genome, *p), text, text_len);
}

int fasim_tfosorted(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len, const char* chr,
	int64_t start_genome, const fasim_params* p, char** text, int64_t* text_len)
{
	return fasim_tfosorted_ex(recs, count, pool, pool_len, chr, start_genome, p, 0, text, text_len);
}

int fasim_tfoclass_ex(const fasim_triplex* recs, int64_t count, int32_t level, const char* chr, int64_t start_genome,
	int64_t dna_len, const char* rna_name, const fasim_params* p, int32_t flags, char** text, int64_t* text_len)
{
	if ((count > 0 && !recs) || !chr || !rna_name || !p || !text || !text_len || count < 0 || level < 1 || level > 5)
		return fail(nullptr, FASIM_E_ARG, "bad arguments");
	std::vector<HostTriplex> list;
	const int rc = records_to_list(recs, count, nullptr, 0, p, start_genome, flags, list);
	if (rc != FASIM_OK) return rc;
	cluster_triplex(p->cDistance, p->cLength, list);
	return text_out(tfoclass_text(list, level, chr, (long)start_genome, (long)dna_len, rna_name, *p), text, text_len);
}

int fasim_tfoclass(const fasim_triplex* recs, int64_t count, int32_t level, const char* chr, int64_t start_genome,
	int64_t dna_len, const char* rna_name, const fasim_params* p, char** text, int64_t* text_len)
{
	return fasim_tfoclass_ex(recs, count, level, chr, start_genome, dna_len, rna_name, p, 0, text, text_len);
}

int fasim_tail_outputs(const fasim_triplex* recs, int64_t count, const char* pool, int64_t pool_len, const char* chr,
	int64_t start_genome, int64_t dna_len, const char* rna_name, const fasim_params* p, int32_t flags,
	char** tfosorted, int64_t* tfosorted_len, char** class1, int64_t* class1_len, char** class2, int64_t* class2_len)
{
	if ((count > 0 && (!recs || !pool)) || !chr || !rna_name || !p || count < 0 || !tfosorted || !tfosorted_len || !class1 || !class1_len ||
		!class2 || !class2_len) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*tfosorted = *class1 = *class2 = nullptr;
	std::vector<HostTriplex> list;
	int rc = records_to_list(recs, count, pool, pool_len, p, start_genome, flags, list);
	if (rc != FASIM_OK) return rc;
	// one clustering serves the three files (tfosorted_text clusters and orders the list; print_cluster only reads classes)
	rc = text_out(tfosorted_text(list, chr, (long)start_genome, *p), tfosorted, tfosorted_len);
	if (rc == FASIM_OK) rc = text_out(tfoclass_text(list, 1, chr, (long)start_genome, (long)dna_len, rna_name, *p), class1, class1_len);
	if (rc == FASIM_OK) rc = text_out(tfoclass_text(list, 2, chr, (long)start_genome, (long)dna_len, rna_name, *p), class2, class2_len);
	if (rc != FASIM_OK) { free(*tfosorted); free(*class1); free(*class2); *tfosorted = *class1 = *class2 = nullptr; }
	return rc;
}

void fasim_upper_case(char* seq, int64_t n)
{
	if (!seq) return;
	for (int64_t i = 0; i < n; i++) { const char c = seq[i]; if (c >= 'a' && c <= 'z') seq[i] = (char)(c - 32); }
}

} // extern "C"

