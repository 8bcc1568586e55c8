// fasim-longtarget_amd/csrc/engine_site_counts.cpp -- sites per threshold with dinucleotide controls:
// fasim_scan_records_site_counts, the host half of k_hist_pairs (the pairs across slice borders and zone borders, the zones, skipped
// segments), the merge of shards, the dinucleotide shuffle, the threshold and the table.
//
// k_hist_pairs (hist_pairs.hip) counts the positions that one segment alone covers and the pairs of neighbours among them that lie
// in one slice.  Everything else is a chain per boundary of a record: the position before the zone, the zone, the position after it.
// A side of a boundary is counted alone when it comes in (its half of the chain, with the values of its segment); when the other
// side is there, both come out again and the chain of the element-wise maximum goes in (book_meet).  That is the whole protocol,
// for the batches of a call under the query's mutex and for the shards of fasim_site_counts_merge alike; a side whose partner never
// comes is what the result carries as a pending edge.
//
// With 2 * overlapLength == cutLength a segment between two others has no interior: its two zones touch, and the pair between them
// depends on both boundaries.  It is counted in the chain of the head zone (link 2 on side 1: `nb` is the first position of the tail
// zone) and only referenced by the tail zone (link 2 on side 0: `nb` is the last position of the head zone, left out of what that
// side counts alone).  When one of the two boundaries is resolved, the `nb` of the other side is set to the resolved value.
#include "engine.h"

namespace {

fasim_site_counts* counts_alloc()
{
	fasim_site_counts* s = (fasim_site_counts*)calloc(1, sizeof(fasim_site_counts));
	if (!s) return nullptr;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
		s->n[c] = (int64_t*)calloc(FASIM_HIST_BINS, sizeof(int64_t));
		s->pairs[c] = (int64_t*)calloc(FASIM_HIST_BINS, sizeof(int64_t));
		if (!s->n[c] || !s->pairs[c]) { fasim_site_counts_free(s); return nullptr; }
	}
	return s;
}

void book_bind(PairBook& B, fasim_site_counts* s) { for (int c = 0; c < 4; c++) { B.n[c] = s->n[c]; B.pairs[c] = s->pairs[c]; } }

inline int bin_of(int v) { return std::min(v, FASIM_HIST_BINS - 1); }
inline int side_value(const PairSide* s, int c, int32_t i) { return s && !s->v.empty() ? bin_of(s->v[(size_t)c * (size_t)s->len + (size_t)i]) : 0; }

// Counts (sign +1) or takes out (sign -1) the chain of a boundary: nb of side 0, the zone, nb of side 1, with the element-wise
// maximum of the sides that are given.  `ref_before`: a side 0 of link 2 brings its nb too (see the head of the file).
void chain(PairBook& B, const PairSide* s0, const PairSide* s1, int64_t sign, bool ref_before)
{
	const int32_t len = s0 ? s0->len : s1->len;
	const bool before = s0 && (s0->link == 1 || (s0->link == 2 && ref_before)), after = s1 && s1->link != 0;
	for (int c = 0; c < 4; c++) {
		int prev = before ? bin_of(s0->nb[c]) : -1;
		for (int32_t i = 0; i < len; i++) {
			const int x = std::max(side_value(s0, c, i), side_value(s1, c, i));
			B.n[c][x] += sign;
			if (prev >= 0) B.pairs[c][std::min(prev, x)] += sign;
			prev = x;
		}
		if (after && prev >= 0) B.pairs[c][std::min(prev, bin_of(s1->nb[c]))] += sign;
	}
	const int64_t links = (int64_t)before + len + (int64_t)after;
	B.positions += sign * len;
	B.npairs += sign * std::max<int64_t>(0, links - 1);
}

// a side comes in; count: it has not been counted yet.  false: the side is there already
bool book_add(PairBook& B, const HistEdgeKey& key, PairSide&& side, bool count)
{
	if (B.open.count(key)) return false;
	if (count) { if (key.side == 0) chain(B, &side, nullptr, 1, false); else chain(B, nullptr, &side, 1, false); }
	B.open.emplace(key, std::move(side));
	return true;
}

// The two sides of boundary (rec, b) meet, if both are there.  false: they have different lengths
bool book_meet(PairBook& B, int32_t rec, int64_t b)
{
	auto i0 = B.open.find(HistEdgeKey{ rec, b, 0 }), i1 = B.open.find(HistEdgeKey{ rec, b, 1 });
	if (i0 == B.open.end() || i1 == B.open.end()) return true;
	const PairSide& s0 = i0->second; const PairSide& s1 = i1->second;
	if (s0.len != s1.len) return false;
	chain(B, &s0, nullptr, -1, true);
	chain(B, nullptr, &s1, -1, true);
	chain(B, &s0, &s1, 1, true);
	// the zones that touch this one inside a segment without interior see the resolved values from now on
	if (s0.len > 0) {
		if (s0.link == 2) {
			auto o = B.open.find(HistEdgeKey{ rec, b - 1, 1 });
			if (o != B.open.end()) for (int c = 0; c < 4; c++) o->second.nb[c] = (uint16_t)std::max(side_value(&s0, c, 0), side_value(&s1, c, 0));
		}
		if (s1.link == 2) {
			auto o = B.open.find(HistEdgeKey{ rec, b + 1, 0 });
			if (o != B.open.end()) for (int c = 0; c < 4; c++) o->second.nb[c] = (uint16_t)std::max(side_value(&s0, c, s0.len - 1), side_value(&s1, c, s0.len - 1));
		}
	}
	B.open.erase(i0); B.open.erase(i1);
	return true;
}

// the sides left in the book into s->pending (the map is ordered by key)
bool counts_set_pending(fasim_site_counts* s, const PairBook& B)
{
	s->npending = 0;
	s->pending = (fasim_site_counts_edge*)calloc(std::max<size_t>(1, B.open.size()), sizeof(fasim_site_counts_edge));
	if (!s->pending) return false;
	for (const auto& kv : B.open) {
		fasim_site_counts_edge& e = s->pending[s->npending];
		e.record = kv.first.rec; e.boundary = kv.first.boundary; e.side = kv.first.side; e.len = kv.second.len; e.link = kv.second.link;
		memcpy(e.nb, kv.second.nb, sizeof e.nb);
		e.v = (uint16_t*)calloc(std::max<size_t>(1, (size_t)4 * (size_t)e.len), sizeof(uint16_t));
		if (!e.v) return false;
		s->npending++;
		if (!kv.second.v.empty()) memcpy(e.v, kv.second.v.data(), (size_t)4 * (size_t)e.len * sizeof(uint16_t));
	}
	return true;
}

} // namespace

// As HistReq::fold, with k_hist_pairs: the counters of the values 0 .. qtop[q] of the positions and of the pairs, the zones (one
// position longer each), the first and last values of every slice and the saturation flags of the batch.
int SiteCountsReq::fold(fasim_engine* E, BatchCtx& C, int q) const
{
	const SiteCountsReq& sr = *this;
	const int nu = C.B.nunit;
	int rc; hipError_t he;
	const int zmax = hist_zone_table(C, sr.step, sr.overlap, sr.rec_nseg);
	C.hist_zstride = (zmax + 1 + 7) & ~7; C.hist_top = sr.qtop[(size_t)q];
	const size_t nzone = (size_t)C.nseg * 8 * (size_t)C.hist_zstride, nborder = (size_t)C.nseg * (size_t)C.track_nchunk * 8;
	const size_t ntop = (size_t)std::min(C.hist_top, HIST_BINS - 1) + 1, nbytes = (size_t)4 * HIST_BINS * sizeof(uint32_t);
	if (E->hist.ensure(nbytes) != hipSuccess || E->hist_pairs.ensure(nbytes) != hipSuccess || E->hist_zones.ensure(nzone * sizeof(uint16_t)) != hipSuccess ||
		E->hist_border.ensure(std::max<size_t>(1, nborder) * sizeof(uint16_t)) != hipSuccess || E->hist_sat.ensure((size_t)nu) != hipSuccess) {
		(void)hipGetLastError();
		return fail(E, FASIM_E_NOMEM, "site counts: no device memory for the counters, %zu zone values and %zu border values of a batch", nzone, nborder);
	}
	rc = upload(E, E->hist_zone, C.hist_zone.data(), sizeof(int32_t) * 2 * (size_t)C.nseg); if (rc) return rc;
	HIPOK(hipMemsetAsync(E->hist.p, 0, nbytes, E->st));
	HIPOK(hipMemsetAsync(E->hist_pairs.p, 0, nbytes, E->st));
	rc = sat_begin(E, E->hist_sat, (size_t)nu); if (rc) return rc;
	HistPairsLaunch H;
	class_fold_fill(H, E, C, E->hist_sat);
	H.zone = E->hist_zone.as<int32_t>(); H.zstride = C.hist_zstride; H.hist = E->hist.as<uint32_t>(); H.zones = E->hist_zones.as<uint16_t>();
	H.pairs = E->hist_pairs.as<uint32_t>(); H.border = E->hist_border.as<uint16_t>();
	{ TimedScope ts(E, 4); he = launch_hist_pairs(H, E->st); }
	if (he != hipSuccess) return fail(E, FASIM_E_HIP, "hist pairs launch failed: %s", hipGetErrorString(he));
	try { C.hist.resize(4 * ntop); C.hist_pairs.resize(4 * ntop); C.hist_zones.resize(nzone); C.hist_border.resize(nborder); C.hist_sat.resize((size_t)nu); }
	catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	for (int c = 0; c < 4; c++) {
		HIPOK(hipMemcpyAsync(C.hist.data() + (size_t)c * ntop, E->hist.as<uint32_t>() + (size_t)c * HIST_BINS, ntop * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
		HIPOK(hipMemcpyAsync(C.hist_pairs.data() + (size_t)c * ntop, E->hist_pairs.as<uint32_t>() + (size_t)c * HIST_BINS, ntop * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st));
	}
	HIPOK(hipMemcpyAsync(C.hist_zones.data(), E->hist_zones.p, nzone * sizeof(uint16_t), hipMemcpyDeviceToHost, E->st));
	if (nborder) HIPOK(hipMemcpyAsync(C.hist_border.data(), E->hist_border.p, nborder * sizeof(uint16_t), hipMemcpyDeviceToHost, E->st));
	return sat_end(E, E->hist_sat, C.hist_sat);
}

// the batch's counters, slice borders, zones and skipped segments [b0, b1) of the call's segment table into the book of query q
void SiteCountsReq::merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q)
{
	SiteCountsReq& sr = *this;
	std::lock_guard<std::mutex> g(sr.mu[(size_t)q]);
	PairBook& B = sr.book[(size_t)q];
	if (C.nseg > 0) {
		const size_t ntop = (size_t)C.hist_top + 1;
		for (int c = 0; c < 4; c++) for (size_t v = 0; v < ntop; v++) { B.n[c][v] += C.hist[(size_t)c * ntop + v]; B.pairs[c][v] += C.hist_pairs[(size_t)c * ntop + v]; }
		for (uint8_t f : C.hist_sat) sr.sat[(size_t)q] += f;
		sr.units[(size_t)q] += C.B.nunit;
	}
	int k = 0;      // next kept segment of the batch
	for (int64_t s = b0; s < b1; s++) {
		const int32_t rec = T.rec[(size_t)s], L = T.len[(size_t)s];
		const int64_t i = T.idx[(size_t)s], nseg = sr.rec_nseg[(size_t)rec];
		const bool kept = k < C.nseg && C.srec[(size_t)k] == rec && C.sidx[(size_t)k] == i;
		int32_t h, t;
		hist_zone_bounds(sr.step, sr.overlap, i, L, nseg, &h, &t);
		// the interior: t - h positions and the t - h - 1 pairs among them, of which the kernel left out those across a slice border
		B.positions += t - h; B.npairs += std::max(0, t - h - 1);
		if (!kept) for (int c = 0; c < 4; c++) { B.n[c][0] += t - h; B.pairs[c][0] += std::max(0, t - h - 1); }      // a skipped segment: potential 0
		else {
			const uint16_t* bd = C.hist_border.data() + (size_t)k * (size_t)C.track_nchunk * 8;
			for (int32_t P0 = TRACK_CHUNK, ch = 1; P0 < L; P0 += TRACK_CHUNK, ch++) {
				if (P0 - 1 < h || P0 >= t) continue;
				for (int c = 0; c < 4; c++) B.pairs[c][bin_of(std::min(bd[(size_t)(ch - 1) * 8 + 4 + c], bd[(size_t)ch * 8 + c]))]++;
			}
		}
		const uint16_t* zsrc = kept ? C.hist_zones.data() + (size_t)k * 8 * (size_t)C.hist_zstride : nullptr;
		const int zs = C.hist_zstride;
		bool have[2] = { i > 0, i + 1 < nseg };
		for (int z = 0; z < 2; z++) {
			if (!have[z]) continue;
			// the head zone is side 1 of boundary i - 1 (slots 0 .. h - 1, then the position behind it), the tail zone side 0 of
			// boundary i (the position ahead of it, then slots 1 .. L - t)
			PairSide side; side.len = z == 0 ? h : L - t;
			if (z == 0) side.link = h >= L ? 0 : h < t ? 1 : 2;
			else side.link = t - 1 >= h ? 1 : 2;
			if (kept) {
				side.v.resize((size_t)4 * (size_t)side.len);
				const uint16_t* src = zsrc + (size_t)z * 4 * (size_t)zs;
				for (int c = 0; c < 4; c++) {
					if (side.len) memcpy(side.v.data() + (size_t)c * side.len, src + (size_t)c * zs + (z == 0 ? 0 : 1), (size_t)side.len * sizeof(uint16_t));
					if (side.link) side.nb[c] = src[(size_t)c * zs + (z == 0 ? h : 0)];
				}
			}
			(void)book_add(B, HistEdgeKey{ rec, z == 0 ? i - 1 : i, z == 0 ? 1 : 0 }, std::move(side), true);
		}
		if (have[0]) (void)book_meet(B, rec, i - 1);
		if (have[1]) (void)book_meet(B, rec, i);
		if (kept) k++;
	}
}

extern "C" {

void fasim_site_counts_free(fasim_site_counts* s)
{
	if (!s) return;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) { free(s->n[c]); free(s->pairs[c]); }
	if (s->pending) for (int64_t k = 0; k < s->npending; k++) free(s->pending[k].v);
	free(s->pending);
	free(s);
}

} // extern "C"

// the request of a call of `nquery` queries over `nrec` records; false: out of memory (outs is cleared)
bool site_counts_req_init(SiteCountsReq& sr, fasim_site_counts** outs, int nquery, const int32_t* qlens, const int64_t* rec_len, int nrec, const fasim_params& p, bool only)
{
	sr.only = only; sr.step = p.cutLength - p.overlapLength; sr.overlap = p.overlapLength;
	sr.rec_nseg.resize((size_t)nrec);
	for (int r = 0; r < nrec; r++) sr.rec_nseg[(size_t)r] = fasim_segment_count(rec_len[r], &p);
	sr.units.assign((size_t)nquery, 0); sr.sat.assign((size_t)nquery, 0);
	sr.book.resize((size_t)nquery); sr.mu.reset(new std::mutex[(size_t)nquery]);
	for (int q = 0; q < nquery; q++) outs[q] = nullptr;
	for (int q = 0; q < nquery; q++) {
		// the potential is at most five points per row of the query, pad rows included
		sr.qtop.push_back((int32_t)std::min<int64_t>(FASIM_HIST_BINS - 1, (int64_t)5 * 16 * ((qlens[q] + 15) / 16)));
		outs[q] = counts_alloc();
		if (!outs[q]) { for (int k = 0; k < q; k++) { fasim_site_counts_free(outs[k]); outs[k] = nullptr; } return false; }
		book_bind(sr.book[(size_t)q], outs[q]);
	}
	return true;
}

// the request's totals and pending edges into the call's results
int site_counts_req_finish(fasim_engine* E, SiteCountsReq& sr, fasim_site_counts** outs, int nquery)
{
	for (int q = 0; q < nquery; q++) {
		fasim_site_counts* s = outs[q];
		const PairBook& B = sr.book[(size_t)q];
		s->positions = B.positions; s->npairs = B.npairs; s->units = sr.units[(size_t)q]; s->saturated_units = sr.sat[(size_t)q];
		if (!counts_set_pending(s, B)) return fail(E, FASIM_E_NOMEM, "out of memory");
	}
	return FASIM_OK;
}

extern "C" {

int fasim_scan_records_site_counts(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_result** out_results, fasim_site_counts** out_counts, fasim_scan_stats* totals)
{
	if (!E) return fail(nullptr, FASIM_E_ARG, "null engine");
	if (!out_counts) return fail(E, FASIM_E_ARG, "bad arguments");
	RecordSet rs;
	int rc = check_records_args(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, pp, true, rs);
	if (rc) return rc;
	rec_off = rs.rec_off; rec_len = rs.rec_len;
	const int nquery = std::max(1, nq);
	const size_t nout = (size_t)nquery * (size_t)nrec;
	rc = check_track_source(E, rna_lens, nq, pp, "site counts"); if (rc) return rc;
	if (2 * (int64_t)pp->overlapLength > (int64_t)pp->cutLength)
		return fail(E, FASIM_E_UNSUPPORTED, "site counts need overlapLength (%d) of at most half of cutLength (%d): a base would lie in three segments", pp->overlapLength, pp->cutLength);
	if (out_results) for (size_t o = 0; o < nout; o++) out_results[o] = nullptr;
	std::vector<int32_t> qlens;
	for (int q = 0; q < nquery; q++) qlens.push_back(nq == 0 ? E->m : rna_lens[q]);
	SiteCountsReq sr;
	try {
		if (!site_counts_req_init(sr, out_counts, nquery, qlens.data(), rec_len, nrec, *pp, out_results == nullptr)) return fail(E, FASIM_E_NOMEM, "out of memory");
	} catch (const std::bad_alloc&) { return fail(E, FASIM_E_NOMEM, "out of memory"); }
	auto drop = [&]() {
		for (int q = 0; q < nquery; q++) { fasim_site_counts_free(out_counts[q]); out_counts[q] = nullptr; }
		if (out_results) for (size_t o = 0; o < nout; o++) { fasim_result_free(out_results[o]); out_results[o] = nullptr; }
	};
	OwnResults res(out_results, nout);
	rc = scan_records_core(E, rnas, rna_lens, nq, dna, rec_off, rec_len, nrec, seg_first, seg_count, pp, res.outs, totals, { &sr });
	if (rc) { drop(); return rc; }
	try { rc = site_counts_req_finish(E, sr, out_counts, nquery); } catch (const std::bad_alloc&) { rc = fail(E, FASIM_E_NOMEM, "out of memory"); }
	if (rc) { drop(); return rc; }
	return FASIM_OK;
}

int fasim_site_counts_merge(const fasim_site_counts* const* parts, int32_t nparts, fasim_site_counts** out)
{
	if (!parts || nparts < 1 || !out) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr;
	for (int k = 0; k < nparts; k++) {
		if (!parts[k] || parts[k]->npending < 0 || (parts[k]->npending > 0 && !parts[k]->pending)) return fail(nullptr, FASIM_E_ARG, "bad site counts %d", k);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) if (!parts[k]->n[c] || !parts[k]->pairs[c]) return fail(nullptr, FASIM_E_ARG, "bad site counts %d", k);
		for (int64_t i = 0; i < parts[k]->npending; i++) {
			const fasim_site_counts_edge& e = parts[k]->pending[i];
			if (e.len < 0 || (e.len > 0 && !e.v) || (e.side != 0 && e.side != 1) || e.link < 0 || e.link > 2) return fail(nullptr, FASIM_E_ARG, "site counts %d: bad pending edge %lld", k, (long long)i);
		}
	}
	fasim_site_counts* s = counts_alloc();
	if (!s) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	try {
		PairBook B;
		book_bind(B, s);
		std::vector<std::pair<int32_t, int64_t>> bounds;
		for (int k = 0; k < nparts; k++) {
			const fasim_site_counts& p = *parts[k];
			B.positions += p.positions; B.npairs += p.npairs; s->units += p.units; s->saturated_units += p.saturated_units;
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) for (int v = 0; v < FASIM_HIST_BINS; v++) { s->n[c][v] += p.n[c][v]; s->pairs[c][v] += p.pairs[c][v]; }
			for (int64_t i = 0; i < p.npending; i++) {
				const fasim_site_counts_edge& e = p.pending[i];
				PairSide side; side.len = e.len; side.link = e.link;
				memcpy(side.nb, e.nb, sizeof side.nb);
				side.v.assign(e.v, e.v + (size_t)4 * (size_t)e.len);
				if (!book_add(B, HistEdgeKey{ e.record, e.boundary, e.side }, std::move(side), false)) {
					fasim_site_counts_free(s);
					return fail(nullptr, FASIM_E_ARG, "record %d, boundary %lld, side %d is pending in two parts: the parts overlap", e.record, (long long)e.boundary, e.side);
				}
				bounds.emplace_back(e.record, e.boundary);
			}
		}
		for (const auto& rb : bounds) {
			if (!book_meet(B, rb.first, rb.second)) {
				fasim_site_counts_free(s);
				return fail(nullptr, FASIM_E_ARG, "record %d, boundary %lld: the two sides have different numbers of positions", rb.first, (long long)rb.second);
			}
		}
		s->positions = B.positions; s->npairs = B.npairs;
		if (!counts_set_pending(s, B)) { fasim_site_counts_free(s); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	} catch (const std::bad_alloc&) { fasim_site_counts_free(s); return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	*out = s;
	return FASIM_OK;
}

int fasim_shuffle_query_dinuc(const char* rna, int32_t m, uint64_t seed, int32_t k, char* out)
{
	if (!rna || !out || m < 1 || k < 1) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (m < 3) { if (out != rna) memmove(out, rna, (size_t)m); return FASIM_OK; }
	try {
		uint64_t s = seed ^ ((uint64_t)k * 0xD1B54A32D192ED03ull);
		auto next = [&s]() {
			s += 0x9E3779B97F4A7C15ull;
			uint64_t z = s;
			z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
			z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
			return z ^ (z >> 31);
		};
		const uint8_t* a = (const uint8_t*)rna;
		const int first = a[0], z = a[m - 1];
		std::vector<uint8_t> succ[256];
		for (int32_t i = 0; i + 1 < m; i++) succ[a[i]].push_back(a[i + 1]);
		// the last edges: a tree towards z
		size_t last[256];
		for (;;) {
			for (int v = 0; v < 256; v++) if (v != z && !succ[v].empty()) last[v] = (size_t)(next() % (uint64_t)succ[v].size());
			bool ok = true;
			for (int v = 0; v < 256 && ok; v++) {
				if (v == z || succ[v].empty()) continue;
				int w = v, steps = 0;
				while (w != z && steps <= 256) { w = succ[w][last[w]]; steps++; }      // (every successor but z has successors of its own)
				ok = w == z;
			}
			if (ok) break;
		}
		for (int v = 0; v < 256; v++) {
			std::vector<uint8_t>& l = succ[v];
			if (l.empty()) continue;
			size_t free_len = l.size();
			if (v != z) {
				const uint8_t e = l[last[v]];
				l.erase(l.begin() + (std::ptrdiff_t)last[v]); l.push_back(e);
				free_len--;
			}
			for (size_t i = free_len; i-- > 1; ) std::swap(l[i], l[(size_t)(next() % (uint64_t)(i + 1))]);
		}
		size_t used[256] = { 0 };
		int w = first;
		out[0] = (char)first;
		for (int32_t i = 1; i < m; i++) { w = succ[w][used[w]++]; out[i] = (char)w; }
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
	return FASIM_OK;
}

} // extern "C"

namespace {

// sites[c][v] = the sum of n[c][w] - pairs[c][w] over w >= v (sites[c][FASIM_HIST_BINS] = 0), summed over `ss`
void sites_of(const fasim_site_counts* const* ss, int32_t ns, std::vector<int64_t>* sites /* [4] */)
{
	for (int c = 0; c < 4; c++) {
		sites[c].assign(FASIM_HIST_BINS + 1, 0);
		for (int v = FASIM_HIST_BINS - 1; v >= 0; v--) {
			int64_t x = 0;
			for (int32_t k = 0; k < ns; k++) x += ss[k]->n[c][v] - ss[k]->pairs[c][v];
			sites[c][(size_t)v] = sites[c][(size_t)v + 1] + x;
		}
	}
}

bool counts_ok(const fasim_site_counts* s) { if (!s) return false; for (int c = 0; c < 4; c++) if (!s->n[c] || !s->pairs[c]) return false; return true; }
inline int64_t all_of(const std::vector<int64_t>* x, int v) { return x[0][(size_t)v] + x[1][(size_t)v] + x[2][(size_t)v] + x[3][(size_t)v]; }

int32_t site_threshold_from(const std::vector<int64_t>* st, const std::vector<int64_t>* cst, int32_t K, double Q)
{
	// from the top: the smallest value with sites above the largest value with sites at which the condition fails
	int32_t best = 0;
	for (int v = FASIM_HIST_BINS - 1; v >= 1; v--) {
		const int64_t g = all_of(st, v);
		if (g <= 0) continue;
		if (!((double)all_of(cst, v) <= Q * (double)K * (double)g)) break;
		best = v;
	}
	return best;
}

} // namespace

extern "C" {

int32_t fasim_site_counts_threshold(const fasim_site_counts* real, const fasim_site_counts* const* controls, int32_t K, double Q)
{
	if (!counts_ok(real) || K < 0 || (K > 0 && !controls) || !(Q > 0.0) || Q > 1.0) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	for (int32_t k = 0; k < K; k++) if (!counts_ok(controls[k])) return fail(nullptr, FASIM_E_ARG, "bad control %d", k);
	try {
		std::vector<int64_t> st[4], cst[4];
		sites_of(&real, 1, st); sites_of(controls, K, cst);
		return site_threshold_from(st, cst, K, Q);
	} catch (const std::bad_alloc&) { return fail(nullptr, FASIM_E_NOMEM, "out of memory"); }
}

int fasim_site_counts_tsv(const fasim_site_counts* real, const fasim_site_counts* const* controls, int32_t K, uint64_t seed, int32_t dinuc, double Q,
	const char* rna_name, char** text, int64_t* text_len)
{
	if (!counts_ok(real) || !rna_name || !text || !text_len || K < 0 || (K > 0 && !controls)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	if (K > 0 && (!(Q > 0.0) || Q > 1.0)) return fail(nullptr, FASIM_E_ARG, "fdr %g lies outside (0, 1]", Q);
	for (int32_t k = 0; k < K; k++) if (!counts_ok(controls[k])) return fail(nullptr, FASIM_E_ARG, "bad control %d", k);
	try {
		std::vector<int64_t> st[4], cst[4];
		sites_of(&real, 1, st); sites_of(controls, K, cst);
		char line[256];
		std::string o = "# fasim site counts lncRNA="; o += rna_name; o += " positions="; o += std::to_string(real->positions);
		if (K > 0) {
			const int32_t v = site_threshold_from(st, cst, K, Q);
			snprintf(line, sizeof line, " controls=%d seed=%llu shuffle=%s fdr=%g min_value=", K, (unsigned long long)seed, dinuc ? "di" : "mono", Q);
			o += line; o += v ? std::to_string(v) : std::string("NA");
		}
		o += "\nvalue";
		for (const char* c : CLASS_NAMES) { o += "\t"; o += c; o += "_sites"; if (K > 0) { o += "\t"; o += c; o += "_ctl_sites"; } }
		o += "\tall_sites";
		if (K > 0) o += "\tall_ctl_sites\tfdr";
		o += "\n";
		int vmax = 0;
		for (int v = FASIM_HIST_BINS - 1; v >= 1 && !vmax; v--) for (int c = 0; c < 4; c++) if (st[c][(size_t)v] > 0 || cst[c][(size_t)v] > 0) vmax = v;
		for (int v = 1; v <= vmax; v++) {
			o += std::to_string(v);
			for (int c = 0; c < 4; c++) {
				o += "\t"; o += std::to_string(st[c][(size_t)v]);
				if (K > 0) { o += "\t"; o += std::to_string(cst[c][(size_t)v]); }
			}
			const int64_t all = all_of(st, v), call = all_of(cst, v);
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
