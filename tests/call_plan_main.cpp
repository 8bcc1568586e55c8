// tests/call_plan_main.cpp -- stand-alone driver of csrc/call_plan.h for tests/test_call_plan_cpu.py: prints the segment table and
// the batches of a call so that the test can compare them with its own restatement of the rules.  Plain host C++, no HIP.
//
//   call_plan_main count CUT OVERLAP LEN...                                 one line per LEN: its segment count
//   call_plan_main table CUT OVERLAP SEG_FIRST SEG_COUNT REC...             the clamped range, rec_first and the table's rows
//   call_plan_main bases CUT OVERLAP SEG_FIRST SEG_COUNT CAP TARGET REC...  the cut by bases of that table: one "chunk b0 b1" per batch
//   call_plan_main fixed SEG_COUNT SEG_BATCH TAPER_PCT                      the fixed / tapered cut
//   call_plan_main @FILE                                                    every line of FILE as one of the above, each behind "# line"
// REC is LEN (the record follows its predecessor in the buffer) or OFF:LEN.
#include "../fasim-longtarget_amd/csrc/call_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

static fasim_params params(const std::string& cut, const std::string& overlap)
{
	fasim_params p;
	memset(&p, 0, sizeof p);
	p.cutLength = atoi(cut.c_str()); p.overlapLength = atoi(overlap.c_str());
	return p;
}

static void records(const std::vector<std::string>& a, size_t from, std::vector<int64_t>& off, std::vector<int64_t>& len)
{
	int64_t next = 0;
	for (size_t k = from; k < a.size(); k++) {
		const size_t colon = a[k].find(':');
		const int64_t o = colon == std::string::npos ? next : atoll(a[k].substr(0, colon).c_str());
		const int64_t n = atoll(a[k].substr(colon == std::string::npos ? 0 : colon + 1).c_str());
		off.push_back(o); len.push_back(n);
		next = o + n;
	}
}

static void print_chunks(const Chunks& c)
{
	for (const auto& x : c) printf("chunk %lld %lld\n", (long long)x.first, (long long)x.second);
}

static int run(const std::vector<std::string>& a)
{
	if (a.empty()) return 2;
	if (a[0] == "count" && a.size() >= 3) {
		const fasim_params p = params(a[1], a[2]);
		for (size_t k = 3; k < a.size(); k++) printf("count %lld\n", (long long)segment_count(atoll(a[k].c_str()), &p));
		return 0;
	}
	if ((a[0] == "table" && a.size() >= 5) || (a[0] == "bases" && a.size() >= 7)) {
		const bool bases = a[0] == "bases";
		const fasim_params p = params(a[1], a[2]);
		std::vector<int64_t> off, len;
		records(a, bases ? 7 : 5, off, len);
		const SegPlan P = segment_plan(off.data(), len.data(), (int)len.size(), atoll(a[3].c_str()), atoll(a[4].c_str()), p);
		if (bases) { print_chunks(cut_by_bases(P.T, P.seg_count, atoll(a[5].c_str()), atoll(a[6].c_str()))); return 0; }
		printf("range %lld %lld %lld\n", (long long)P.seg_first, (long long)P.seg_count, (long long)P.total_bases);
		printf("first");
		for (int64_t f : P.rec_first) printf(" %lld", (long long)f);
		printf("\n");
		for (int64_t s = 0; s < P.T.size(); s++)
			printf("seg %d %lld %lld %d\n", (int)P.T.rec[(size_t)s], (long long)P.T.idx[(size_t)s], (long long)P.T.off[(size_t)s], (int)P.T.len[(size_t)s]);
		return 0;
	}
	if (a[0] == "fixed" && a.size() == 4) { print_chunks(cut_fixed(atoll(a[1].c_str()), atoll(a[2].c_str()), atoi(a[3].c_str()))); return 0; }
	return 2;
}

int main(int argc, char** argv)
{
	if (argc == 2 && argv[1][0] == '@') {
		std::ifstream f(argv[1] + 1);
		if (!f) { fprintf(stderr, "cannot read %s\n", argv[1] + 1); return 2; }
		std::string line;
		while (std::getline(f, line)) {
			std::istringstream is(line);
			std::vector<std::string> a;
			for (std::string w; is >> w; ) a.push_back(w);
			if (a.empty()) continue;
			printf("# %s\n", line.c_str());
			if (run(a)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
		}
		return 0;
	}
	const int rc = run(std::vector<std::string>(argv + 1, argv + argc));
	if (rc) fprintf(stderr, "usage: see the head of tests/call_plan_main.cpp\n");
	return rc;
}
