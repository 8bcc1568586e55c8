// fasim-longtarget_amd/csrc/engine_hist.cpp -- histograms of the per-base potential with shuffled controls:
// fasim_scan_records_hist, the host half of k_hist (zone bounds, the zone protocol between batches, skipped segments), the merge of
// shards, the shuffle of the controls, the threshold and the table.
//
// k_hist (hist.hip) counts the positions that one segment alone covers.  A position in the overlap of two segments counts once, with
// the maximum of the two: the kernel leaves the zone values of every segment, and the worker that brings the second side of a
// boundary counts it (HistReq::merge, under the query's mutex).  A side whose partner lies outside the call's segment range is counted
// alone and travels in the result as a pending edge; fasim_hist_merge takes both sides out again and counts their maximum.
#include "engine.h"

namespace {

fasim_hist* hist_alloc()
{
	fasim_hist* h = (fasim_hist*)calloc(1, sizeof(fasim_hist));
	if (!h) return nullptr;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
		h->n[c] = (int64_t*)calloc(FASIM_HIST_BINS, sizeof(int64_t));
		if (!h->n[c]) { fasim_hist_free(h); return nullptr; }
	}
	return h;
}

// the pending edges of `v` (ordered by key) into h
bool hist_set_pending(fasim_hist* h, const std::vector<std::pair<HistEdgeKey, HistSide>>& v)
{
	h->npending = 0;
	h->pending = (fasim_hist_edge*)calloc(std::max<size_t>(1, v.size()), sizeof(fasim_hist_edge));
	if (!h->pending) return false;
	for (const auto& kv : v) {
		fasim_hist_edge& e = h->pending[h->npending];
		e.record = kv.first.rec; e.boundary = kv.first.boundary; e.side = kv.first.side; e.len = kv.second.len; e.reserved = 0;
		e.v = (uint16_t*)calloc(std::max<size_t>(1, (size_t)4 * (size_t)e.len), sizeof(uint16_t));
		if (!e.v) return false;
		h->npending++;
		if (!kv.second.v.empty()) memcpy(e.v, kv.second.v.data(), (size_t)4 * (size_t)e.len * sizeof(uint16_t));
	}
	return true;
}

// counts (sign +1) or takes out (sign -1) the positions of one side alone, or with `b` the element-wise maximum of two sides
void count_side(int64_t* const* n, const uint16_t* a, const uint16_t* b, int32_t len, int64_t sign)
{
	for (int c = 0; c < 4; c++) {
		for (int32_t i = 0; i < len; i++) {
			const uint16_t x = a ? a[(size_t)c * len + i] : 0, y = b ? b[(size_t)c * len + i] : 0;
			n[c][std::min<int>(std::max(x, y), FASIM_HIST_BINS - 1)] += sign;
		}
	}
}

// One side of a boundary arrives for query q (the query's mutex is held).  Partner outside the call's range: counted alone, pending.
// Otherwise the side waits for its partner, or meets it: the maximum of the two is counted once.
void side_arrives(HistReq& hr, int q, const HistEdgeKey& key, HistSide&& side, bool partner_in_range)
{
	int64_t* const* n = &hr.n[(size_t)q * 4];
	if (!partner_in_range) {
		count_side(n, side.v.empty() ? nullptr : side.v.data(), nullptr, side.len, 1);
		hr.positions[(size_t)q] += side.len;
		hr.pending[(size_t)q].emplace_back(key, std::move(side));
		return;
	}
	HistEdgeKey other = key; other.side ^= 1;
	auto& open = hr.open[(size_t)q];
	auto it = open.find(other);
	if (it == open.end()) { open.emplace(key, std::move(side)); return; }
	const HistSide& o = it->second;
	const int32_t len = std::min(side.len, o.len);      // (equal by construction)
	count_side(n, side.v.empty() ? nullptr : side.v.data(), o.v.empty() ? nullptr : o.v.data(), len, 1);
	hr.positions[(size_t)q] += len;
	open.erase(it);
}

// head-zone end and tail-zone begin of segment i (length L) of a record of `nseg` segments
inline void zone_bounds(const HistReq& hr, int64_t i, int32_t L, int64_t nseg, int32_t* head, int32_t* tail)
{
	hist_zone_bounds(hr.step, hr.overlap, i, L, nseg, head, tail);
}

} // namespace

// The zone bounds of the batch's kept segments into C.hist_zone, and k_hist over the batch's column maxima in E->colmax16 into
// C.hist / C.hist_zones / C.hist_sat: the counters of the values 0 .. qtop[q] per class, the zone values and the saturation flags.
// The copies complete at the next synchronisation of the stream.
int HistReq::fold(fasim_engine* E, BatchCtx& C, int q) const
{
	const HistReq& hr = *this;
	const int nu = C.B.nunit;
	int rc; hipError_t he;
	const int zmax = hist_zone_table(C, hr.step, hr.overlap, hr.rec_nseg);
	C.hist_zstride = (zmax + 7) & ~7; C.hist_top = hr.qtop[(size_t)q];
	const size_t nzone = (size_t)C.nseg * 8 * (size_t)C.hist_zstride;
	const size_t ntop = (size_t)std::min(C.hist_top, HIST_BINS - 1) + 1;
	if (E->hist.ensure((size_t)4 * HIST_BINS * sizeof(uint32_t)) != hipSuccess || E->hist_zones.ensure(std::max<size_t>(1, nzone) * sizeof(uint16_t)) != hipSuccess ||
		E->hist_sat.ensure((size_t)nu) != hipSuccess) {
		(void)hipGetLastError();
		return fail(E, FASIM_E_NOMEM, "histogram: no device memory for the counters and %zu zone values of a batch", nzone);
	}
	rc = upload(E, E->hist_zone, C.hist_zone.data(), sizeof(int32_t) * 2 * (size_t)C.nseg); if (rc) return rc;
	HIPOK(hipMemsetAsync(E->hist.p, 0, (size_t)4 * HIST_BINS * sizeof(uint32_t), E->st));
	rc = sat_begin(E, E->hist_sat, (size_t)nu); if (rc) return rc;
	HistLaunch H;
	class_fold_fill(H, E, C, E->hist_sat);
	H.zone = E->hist_zone.as<int32_t>(); H.zstride = C.hist_zstride; H.hist = E->hist.as<uint32_t>(); H.zones = E->hist_zones.as<uint16_t>();
	{ TimedScope ts(E, 4); he = launch_hist(H, E->st); }
	if (he != hipSuccess) return fail(E, FASIM_E_HIP, "hist launch failed: %s", hipGetErrorString(he));
	try { C.hist.resize(4 * ntop); C.hist_zones.resize(nzone); C.hist_sat.resize((size_t)nu); } catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	for (int c = 0; c < 4; c++)
		HIPOK(hipMemcpyAsync(C.hist.data() + (size_t)c * ntop, E->hist.as<uint32_t>() + (size_t)c * HIST_BINS, ntop * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
	if (nzone) HIPOK(hipMemcpyAsync(C.hist_zones.data(), E->hist_zones.p, nzone * sizeof(uint16_t), hipMemcpyDeviceToHost, E->st));
	return sat_end(E, E->hist_sat, C.hist_sat);
}

// the batch's counters, zones and skipped segments [b0, b1) of the call's segment table into the arrays of query q
void HistReq::merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q)
{
	HistReq& hr = *this;
	std::lock_guard<std::mutex> g(hr.mu[(size_t)q]);
	int64_t* const* n = &hr.n[(size_t)q * 4];
	if (C.nseg > 0) {
		const size_t ntop = (size_t)C.hist_top + 1;
		for (int c = 0; c < 4; c++) for (size_t v = 0; v < ntop; v++) n[c][v] += C.hist[(size_t)c * ntop + v];
		for (uint8_t f : C.hist_sat) hr.sat[(size_t)q] += f;
		hr.units[(size_t)q] += C.B.nunit;
	}
	int k = 0;      // next kept segment of the batch
	for (int64_t s = b0; s < b1; s++) {
		const int32_t rec = T.rec[(size_t)s], L = T.len[(size_t)s];
		const int64_t i = T.idx[(size_t)s];
		const bool kept = k < C.nseg && C.srec[(size_t)k] == rec && C.sidx[(size_t)k] == i;
		int32_t h, t;
		zone_bounds(hr, i, L, hr.rec_nseg[(size_t)rec], &h, &t);
		hr.positions[(size_t)q] += t - h;
		if (!kept) n[0][0] += t - h, n[1][0] += t - h, n[2][0] += t - h, n[3][0] += t - h;      // a skipped segment: potential 0
		for (int z = 0; z < 2; z++) {
			const int32_t len = z == 0 ? h : L - t;
			if (len <= 0) continue;
			HistSide side; side.len = len;
			if (kept) {
				side.v.resize((size_t)4 * len);
				const uint16_t* src = C.hist_zones.data() + ((size_t)k * 2 + z) * 4 * (size_t)C.hist_zstride;
				for (int c = 0; c < 4; c++) memcpy(side.v.data() + (size_t)c * len, src + (size_t)c * C.hist_zstride, (size_t)len * sizeof(uint16_t));
			}
			// the head zone is side 1 of boundary i - 1 (partner: the segment before), the tail zone side 0 of boundary i (the one after)
			const HistEdgeKey key{ rec, z == 0 ? i - 1 : i, z == 0 ? 1 : 0 };
			const bool in_range = z == 0 ? s > 0 : s + 1 < T.size();
			side_arrives(hr, q, key, std::move(side), in_range);
		}
		if (kept) k++;
	}
}

extern "C" {

void fasim_hist_free(fasim_hist* h)
{
	if (!h) return;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) free(h->n[c]);
	if (h->pending) for (int64_t k = 0; k < h->npending; k++) free(h->pending[k].v);
	free(h->pending);
	free(h);
}

} // extern "C"

// the request of a call of `nquery` queries over `nrec` records; false: out of memory (out_hists is cleared)
bool hist_req_init(HistReq& hr, fasim_hist** out_hists, int nquery, const int32_t* qlens, const int64_t* rec_len, int nrec, const fasim_params& p, bool only)
{
	hr.only = only; hr.step = p.cutLength - p.overlapLength; hr.overlap = p.overlapLength;
	hr.rec_nseg.resize((size_t)nrec);
	for (int r = 0; r < nrec; r++) hr.rec_nseg[(size_t)r] = fasim_segment_count(rec_len[r], &p);
	hr.positions.assign((size_t)nquery, 0); hr.units.assign((size_t)nquery, 0); hr.sat.assign((size_t)nquery, 0);
	hr.open.resize((size_t)nquery); hr.pending.resize((size_t)nquery); hr.mu.reset(new std::mutex[(size_t)nquery]);
	for (int q = 0; q < nquery; q++) out_hists[q] = nullptr;
	for (int q = 0; q < nquery; q++) {
		// the potential is at most five points per row of the query, pad rows included
		hr.qtop.push_back((int32_t)std::min<int64_t>(FASIM_HIST_BINS - 1, (int64_t)5 * 16 * ((qlens[q] + 15) / 16)));
		out_hists[q] = hist_alloc();
		if (!out_hists[q]) { for (int k = 0; k < q; k++) { fasim_hist_free(out_hists[k]); out_hists[k] = nullptr; } return false; }
		for (int c = 0; c < 4; c++) hr.n.push_back(out_hists[q]->n[c]);
	}
	return true;
}

// the request's totals and pending edges into the call's results
int hist_req_finish(fasim_engine* E, HistReq& hr, fasim_hist** out_hists, int nquery)
{
	for (int q = 0; q < nquery; q++) {
		if (!hr.open[(size_t)q].empty()) return fail(E, FASIM_E_HIP, "histogram: %zu zone sides of query %d never met their partner", hr.open[(size_t)q].size(), q);
		fasim_hist* h = out_hists[q];
		h->positions = hr.positions[(size_t)q]; h->units = hr.units[(size_t)q]; h->saturated_units = hr.sat[(size_t)q];
		auto& v = hr.pending[(size_t)q];
		std::sort(v.begin(), v.end(), [](const std::pair<HistEdgeKey, HistSide>& a, const std::pair<HistEdgeKey, HistSide>& b) { return a.first < b.first; });
		if (!hist_set_pending(h, v)) return fail(E, FASIM_E_NOMEM, "out of memory");
	}
	return FASIM_OK;
}

extern "C" {

int fasim_scan_records_hist(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_result** out_results, fasim_hist** out_hists, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_hists) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, true, rs);
	if (rc) return rc;
	rec_off = rs.rec_off; rec_len = rs.rec_len;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec;
	rc = check_track_source(E, rna_lens, nq, pp, "histograms of the potential"); if (rc) return rc;
	if (2 * (int64_t)pp->overlapLength > (int64_t)pp->cutLength)
		return fail(E, FASIM_E_UNSUPPORTED, "histograms of the potential need overlapLength (%d) of at most half of cutLength (%d): a base would lie in three segments", pp->overlapLength, pp->cutLength);
	if (out_results) for (size_t o = 0; o < nout; o++) out_results[o] = nullptr;
	std::vector<int32_t> qlens;
	for (int q = 0; q < nquery; q++) qlens.push_back(nq == 0 ? E->m : rna_lens[q]);
	HistReq hr;
	try {
		if (!hist_req_init(hr, out_hists, nquery, qlens.data(), rec_len, nrec, *pp, out_results == nullptr)) return fail(E, FASIM_E_NOMEM, "out of memory");
	} catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	auto drop = [&]() {
		for (int q = 0; q < nquery; q++) { fasim_hist_free(out_hists[q]); out_hists[q] = nullptr; }
		if (out_results) for (size_t o = 0; o < nout; o++) { fasim_result_free(out_results[o]); out_results[o] = nullptr; }
	};
	OwnResults res(out_results, nout);
	rc = scan_records_core(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, res.outs, totals, { &hr });
	if (rc) { drop(); return rc; }
	try { rc = hist_req_finish(E, hr, out_hists, nquery); } catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (rc) { drop(); return rc; }
	return FASIM_OK;
}

int fasim_hist_merge(const fasim_hist* const* parts, int32_t nparts, fasim_hist** out)
{
	if (!parts || nparts < 1 || !out) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr;
	for (int k = 0; k < nparts; k++) {
		if (!parts[k] || parts[k]->npending < 0 || (parts[k]->npending > 0 && !parts[k]->pending)) return fail(nullptr, FASIM_E_ARG, "bad histogram %d", k);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) if (!parts[k]->n[c]) return fail(nullptr, FASIM_E_ARG, "bad histogram %d", k);
		for (int64_t i = 0; i < parts[k]->npending; i++) {
			const fasim_hist_edge& e = parts[k]->pending[i];
			if (e.len < 0 || (e.len > 0 && !e.v) || (e.side != 0 && e.side != 1)) return fail(nullptr, FASIM_E_ARG, "histogram %d: bad pending edge %lld", k, (long long)i);
		}
	}
	fasim_hist* h = hist_alloc();
	if (!h) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	try {
		std::map<HistEdgeKey, const fasim_hist_edge*> open;
		for (int k = 0; k < nparts; k++) {
			h->positions += parts[k]->positions; h->units += parts[k]->units; h->saturated_units += parts[k]->saturated_units;
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) for (int v = 0; v < FASIM_HIST_BINS; v++) h->n[c][v] += parts[k]->n[c][v];
			for (int64_t i = 0; i < parts[k]->npending; i++) {
				const fasim_hist_edge& e = parts[k]->pending[i];
				const HistEdgeKey key{ e.record, e.boundary, e.side };
				if (open.count(key)) { fasim_hist_free(h); return fail(nullptr, FASIM_E_ARG, "record %d, boundary %lld, side %d is pending in two parts: the parts overlap", e.record, (long long)e.boundary, e.side); }
				HistEdgeKey other = key; other.side ^= 1;
				auto it = open.find(other);
				if (it == open.end()) { open.emplace(key, &e); continue; }
				const fasim_hist_edge& o = *it->second;
				if (o.len != e.len) { fasim_hist_free(h); return fail(nullptr, FASIM_E_ARG, "record %d, boundary %lld: the two sides have %d and %d positions", e.record, (long long)e.boundary, o.len, e.len); }
				// what each side counted alone comes out, the maximum of the two goes in
				count_side(h->n, e.v, nullptr, e.len, -1);
				count_side(h->n, o.v, nullptr, e.len, -1);
				count_side(h->n, e.v, o.v, e.len, 1);
				h->positions -= e.len;
				open.erase(it);
			}
		}
		std::vector<std::pair<HistEdgeKey, HistSide>> left;
		for (const auto& kv : open) {
			HistSide s; s.len = kv.second->len;
			s.v.assign(kv.second->v, kv.second->v + (size_t)4 * (size_t)s.len);
			left.emplace_back(kv.first, std::move(s));
		}
		if (!hist_set_pending(h, left)) { fasim_hist_free(h); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	} catch (const std::bad_alloc&) { fasim_hist_free(h); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	*out = h;
	return FASIM_OK;
}

int fasim_shuffle_query(const char* rna, int32_t m, uint64_t seed, int32_t k, char* out)
{
	if (!rna || !out || m < 1 || k < 1) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (out != rna) memmove(out, rna, (size_t)m);
	uint64_t s = seed ^ ((uint64_t)k * 0xD1B54A32D192ED03ull);
	for (int32_t i = m - 1; i >= 1; i--) {
		s += 0x9E3779B97F4A7C15ull;
		uint64_t z = s;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z ^= z >> 31;
		const int32_t j = (int32_t)(z % (uint64_t)(i + 1));
		std::swap(out[i], out[j]);
	}
	return FASIM_OK;
}

} // extern "C"

namespace {

// ge[c][v] = the sum of n[c][w] over w >= v (ge[c][FASIM_HIST_BINS] = 0), summed over `hs`
void hist_ge(const fasim_hist* const* hs, int32_t nh, std::vector<int64_t>* ge /* [4] */)
{
	for (int c = 0; c < 4; c++) {
		ge[c].assign(FASIM_HIST_BINS + 1, 0);
		for (int v = FASIM_HIST_BINS - 1; v >= 0; v--) {
			int64_t x = 0;
			for (int32_t k = 0; k < nh; k++) x += hs[k]->n[c][v];
			ge[c][(size_t)v] = ge[c][(size_t)v + 1] + x;
		}
	}
}

bool hist_ok(const fasim_hist* h) { return h && h->n[0] && h->n[1] && h->n[2] && h->n[3]; }

int32_t threshold_from(const std::vector<int64_t>* ge, const std::vector<int64_t>* cge, int32_t K, double Q)
{
	// from the top: the largest value with counts, and the largest value at which the condition fails
	int32_t vmax = 0, fail_at = 0;
	for (int v = FASIM_HIST_BINS - 1; v >= 1; v--) {
		const int64_t g = ge[0][(size_t)v] + ge[1][(size_t)v] + ge[2][(size_t)v] + ge[3][(size_t)v];
		if (g <= 0) continue;
		if (!vmax) vmax = v;
		const int64_t cg = cge[0][(size_t)v] + cge[1][(size_t)v] + cge[2][(size_t)v] + cge[3][(size_t)v];
		if (!((double)cg <= Q * (double)K * (double)g)) { fail_at = v; break; }
	}
	const int32_t v = fail_at + 1;
	return vmax >= 1 && v <= vmax ? v : 0;
}

} // namespace

extern "C" {

int32_t fasim_hist_threshold(const fasim_hist* real, const fasim_hist* const* controls, int32_t K, double Q)
{
	if (!hist_ok(real) || K < 0 || (K > 0 && !controls) || !(Q > 0.0) || Q > 1.0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	for (int32_t k = 0; k < K; k++) if (!hist_ok(controls[k])) return fail(nullptr, FASIM_E_ARG, "bad control %d", k);
	try {
		std::vector<int64_t> ge[4], cge[4];
		hist_ge(&real, 1, ge); hist_ge(controls, K, cge);
		return threshold_from(ge, cge, K, Q);
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
}

int fasim_hist_tsv(const fasim_hist* real, const fasim_hist* const* controls, int32_t K, uint64_t seed, double Q, const char* rna_name,
	char** text, int64_t* text_len)
{
	if (!hist_ok(real) || !rna_name || !text || !text_len || K < 0 || (K > 0 && !controls)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (K > 0 && (!(Q > 0.0) || Q > 1.0)) return fail(nullptr, FASIM_E_ARG, "fdr %g lies outside (0, 1]", Q);
	for (int32_t k = 0; k < K; k++) if (!hist_ok(controls[k])) return fail(nullptr, FASIM_E_ARG, "bad control %d", k);
	try {
		std::vector<int64_t> ge[4], cge[4];
		hist_ge(&real, 1, ge); hist_ge(controls, K, cge);
		char line[256];
		std::string o = "# fasim potential histogram lncRNA="; o += rna_name; o += " positions="; o += std::to_string(real->positions);
		if (K > 0) {
			const int32_t v = threshold_from(ge, cge, K, Q);
			snprintf(line, sizeof line, " controls=%d seed=%llu fdr=%g min_value=", K, (unsigned long long)seed, Q);
			o += line; o += v ? std::to_string(v) : std::string("NA");
		}
		o += "\nvalue";
		for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "\t"; o += c; o += "_ge"; if (K > 0) { o += "\t"; o += c; o += "_ctl_ge"; } }
		o += "\tall_ge";
		if (K > 0) o += "\tall_ctl_ge\tfdr";
		o += "\n";
		int vmax = 0;
		for (int v = FASIM_HIST_BINS - 1; v >= 1 && !vmax; v--) for (int c = 0; c < 4; c++) if (ge[c][(size_t)v] > 0 || cge[c][(size_t)v] > 0) vmax = v;
		for (int v = 1; v <= vmax; v++) {
			o += std::to_string(v);
			int64_t all = 0, call = 0;
			for (int c = 0; c < 4; c++) {
				o += "\t"; o += std::to_string(real->n[c][v]); o += "\t"; o += std::to_string(ge[c][(size_t)v]);
				if (K > 0) { o += "\t"; o += std::to_string(cge[c][(size_t)v]); }
				all += ge[c][(size_t)v]; call += cge[c][(size_t)v];
			}
			o += "\t"; o += std::to_string(all);
			if (K > 0) {
				o += "\t"; o += std::to_string(call);
				if (all > 0) { snprintf(line, sizeof line, "\t%.6g", (double)call / ((double)K * (double)all)); o += line; }
				else o += "\tNA";
			}
			o += "\n";
		}
		return text_out(o, text, text_len);
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
}

} // extern "C"
