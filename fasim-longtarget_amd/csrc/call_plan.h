// fasim-longtarget_amd/csrc/call_plan.h -- the pure part of a call's frame: how a record set is cut into segments and the segments
// into batches.  No HIP and no engine: only include/fasim_hip.h and the standard library, so a plain host compiler takes it
// (tests/call_plan_main.cpp drives it).  The frame around it -- argument checks, workers, requests -- is in engine.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/fasim_hip.h"

// the four strand classes in the order of FASIM_TRACK_CLASSES, as every table and track names them
inline constexpr const char* const CLASS_NAMES[FASIM_TRACK_CLASSES] = { "ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus" };

// cutSequence (fastsim.h:71-90): pos += cut - overlap while pos < size
inline int64_t segment_count(int64_t dna_len, const fasim_params* p)
{
	if (dna_len <= 0 || !p || p->cutLength - p->overlapLength <= 0) return 0;
	const int64_t step = p->cutLength - p->overlapLength;
	return (dna_len + step - 1) / step;
}

// Segments of one scan call, numbered globally record after record (a single-record scan is the one-record case).  Entry k
// is the k-th segment of the call's selected range: its record, its index within the record, its offset in the call's DNA
// buffer and its length.
struct SegTable {
	std::vector<int32_t> rec, len;
	std::vector<int64_t> idx, off;
	int64_t size() const { return (int64_t)rec.size(); }
};

// The selected range of a call's global segment list: rec_first[r] is the global number of record r's first segment
// (rec_first[nrec]: all segments), [seg_first, seg_first + seg_count) the range clamped to the list.
struct SegRange {
	std::vector<int64_t> rec_first;
	int64_t seg_first = 0, seg_count = 0;
};
inline SegRange segment_range(const int64_t* rec_len, int nrec, int64_t seg_first, int64_t seg_count, const fasim_params& p)
{
	SegRange R;
	R.rec_first.assign((size_t)nrec + 1, 0);
	for (int r = 0; r < nrec; r++) R.rec_first[(size_t)r + 1] = R.rec_first[(size_t)r] + segment_count(rec_len[r], &p);
	const int64_t nseg_all = R.rec_first[(size_t)nrec];
	if (seg_first < 0) seg_first = 0;
	if (seg_count < 0 || seg_first + seg_count > nseg_all) seg_count = std::max<int64_t>(0, nseg_all - seg_first);
	R.seg_first = seg_first; R.seg_count = seg_count;
	return R;
}

// the range with its segment table (cutSequence() of every record) and the bases of the table's segments
struct SegPlan : SegRange {
	SegTable T;
	int64_t total_bases = 0;
};
inline SegPlan segment_plan(const int64_t* rec_off, const int64_t* rec_len, int nrec, int64_t seg_first, int64_t seg_count, const fasim_params& p)
{
	SegPlan P;
	static_cast<SegRange&>(P) = segment_range(rec_len, nrec, seg_first, seg_count, p);
	if (P.seg_count <= 0) return P;
	const int64_t step = p.cutLength - p.overlapLength;
	SegTable& T = P.T;
	T.rec.reserve((size_t)P.seg_count); T.len.reserve((size_t)P.seg_count); T.idx.reserve((size_t)P.seg_count); T.off.reserve((size_t)P.seg_count);
	int r = (int)(std::upper_bound(P.rec_first.begin(), P.rec_first.end(), P.seg_first) - P.rec_first.begin()) - 1;
	for (int64_t g = P.seg_first; g < P.seg_first + P.seg_count; g++) {
		while (g >= P.rec_first[(size_t)r + 1]) r++;
		const int64_t i = g - P.rec_first[(size_t)r], pos = i * step;
		const int len = (int)std::min<int64_t>(p.cutLength, rec_len[r] - pos);
		T.rec.push_back(r); T.idx.push_back(i); T.off.push_back(rec_off[r] + pos); T.len.push_back(len);
		P.total_bases += len;
	}
	return P;
}

// batches of a call: ranges [first, second) of the segment table (local indices; a batch may cross records)
typedef std::vector<std::pair<int64_t, int64_t>> Chunks;

// A record set is cut by bases, not by segments: a batch of short records' segments would otherwise carry a fraction of a batch's
// work for the whole fixed latency of its chain of launches.  A batch closes once it holds `cap` segments or `target` bases.
inline Chunks cut_by_bases(const SegTable& T, int64_t seg_count, int64_t cap, int64_t target)
{
	Chunks chunks;
	int64_t b0 = 0, bases = 0;
	for (int64_t s = 0; s < seg_count; s++) {
		bases += T.len[(size_t)s];
		if (s + 1 - b0 >= cap || bases >= target) { chunks.push_back({ b0, s + 1 }); b0 = s + 1; bases = 0; }
	}
	if (b0 < seg_count) chunks.push_back({ b0, seg_count });
	return chunks;
}

// Batches of seg_batch segments; the last taper_pct percent of the segments go in half-size batches, so that the workers do not
// all finish their last batch at the same moment (shorter drain at the end of a scan).
inline Chunks cut_fixed(int64_t seg_count, int64_t seg_batch, int taper_pct)
{
	Chunks chunks;
	int64_t b0 = 0; const int64_t b_end = seg_count;
	const int64_t taper_from = b_end - seg_count * taper_pct / 100;
	while (b0 < b_end) {
		int64_t len = (taper_pct > 0 && b0 >= taper_from) ? std::max<int64_t>(1, seg_batch / 2) : seg_batch;
		len = std::min(len, b_end - b0);
		chunks.push_back({ b0, b0 + len });
		b0 += len;
	}
	return chunks;
}
