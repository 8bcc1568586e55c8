// BED intervals for region scans (`fasim --regions`, read_bed() of the Python package): fasim_read_bed (include/fasim_hip.h).
// Pure host code.  One parser serves the CLI and Python, so both refuse the same files with the same messages.
#include "engine.h"

#include <cerrno>
#include <fstream>
#include <set>
#include <utility>

namespace {

struct BedRow { int64_t line, start, end; std::string chrom, name; };

// whole token an integer (optional sign, decimal digits, no overflow)
bool parse_int(const std::string& s, int64_t& v)
{
	if (s.empty()) return false;
	errno = 0;
	char* end = nullptr;
	const long long x = strtoll(s.c_str(), &end, 10);
	if (errno || end != s.c_str() + s.size() || !(isdigit((unsigned char)s.back()))) return false;
	v = (int64_t)x;
	return true;
}

std::vector<std::string> split_ws(const std::string& line)
{
	std::vector<std::string> f;
	size_t i = 0;
	while (i < line.size()) {
		while (i < line.size() && isspace((unsigned char)line[i])) i++;
		const size_t b = i;
		while (i < line.size() && !isspace((unsigned char)line[i])) i++;
		if (i > b) f.emplace_back(line, b, i - b);
	}
	return f;
}

}  // namespace

int fasim_read_bed(const char* path, fasim_region** out, int64_t* n)
{
	if (!path || !out || !n) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr; *n = 0;
	std::ifstream in(path);
	if (!in) return fail(nullptr, FASIM_E_ARG, "cannot read BED file %s", path);
	std::vector<BedRow> rows;
	std::string line;
	int64_t ln = 0;
	size_t strbytes = 0;
	while (std::getline(in, line)) {
		ln++;
		const std::vector<std::string> f = split_ws(line);
		if (f.empty() || f[0][0] == '#' || f[0] == "track" || f[0] == "browser") continue;
		if (f.size() < 3) return fail(nullptr, FASIM_E_ARG, "%s line %lld: fewer than 3 columns", path, (long long)ln);
		BedRow r;
		r.line = ln; r.chrom = f[0];
		if (!parse_int(f[1], r.start)) return fail(nullptr, FASIM_E_ARG, "%s line %lld: start '%s' is not an integer", path, (long long)ln, f[1].c_str());
		if (!parse_int(f[2], r.end)) return fail(nullptr, FASIM_E_ARG, "%s line %lld: end '%s' is not an integer", path, (long long)ln, f[2].c_str());
		if (r.start < 0) return fail(nullptr, FASIM_E_ARG, "%s line %lld: start %lld < 0", path, (long long)ln, (long long)r.start);
		if (r.end <= r.start) return fail(nullptr, FASIM_E_ARG, "%s line %lld: end %lld <= start %lld", path, (long long)ln, (long long)r.end, (long long)r.start);
		if (r.end - r.start > 0x7fffffffll)
			return fail(nullptr, FASIM_E_ARG, "%s line %lld: interval of %lld nt is longer than 2^31 - 1 (one record's limit)", path, (long long)ln, (long long)(r.end - r.start));
		r.name = f.size() >= 4 ? f[3] : r.chrom + "_" + std::to_string(r.start + 1) + "_" + std::to_string(r.end);
		rows.push_back(std::move(r));
	}
	// the output stem is <name>-<lnc>-<f1 stem>.<chrom>: a (name, chrom) pair seen before gets "_<line>" until it is unique
	std::set<std::pair<std::string, std::string>> seen;
	for (BedRow& r : rows) {
		while (!seen.insert({ r.name, r.chrom }).second) r.name += "_" + std::to_string(r.line);
		strbytes += r.chrom.size() + r.name.size() + 2;
	}
	// one block: the records, then their strings (a single fasim_free releases both)
	const size_t head = rows.size() * sizeof(fasim_region);
	char* block = (char*)malloc(head + strbytes + 1);
	if (!block) return fail(nullptr, FASIM_E_NOMEM, "out of host memory for %zu BED intervals", rows.size());
	fasim_region* reg = (fasim_region*)block;
	char* s = block + head;
	for (size_t k = 0; k < rows.size(); k++) {
		const BedRow& r = rows[k];
		reg[k].line = r.line; reg[k].start = r.start; reg[k].end = r.end;
		memcpy(s, r.chrom.c_str(), r.chrom.size() + 1); reg[k].chrom = s; s += r.chrom.size() + 1;
		memcpy(s, r.name.c_str(), r.name.size() + 1); reg[k].name = s; s += r.name.size() + 1;
	}
	*out = reg; *n = (int64_t)rows.size();
	return FASIM_OK;
}
