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

// ---- variants (`fasim --variants`, read_vcf() of the Python package): fasim_read_vcf ------------------------------------------------
namespace {

struct VcfRow { int64_t line, pos; std::string chrom, id, ref, alt; bool usable; };

// an allele fasim_score_variants takes: 1 .. FASIM_MAX_ALLELE letters of ACGTN (symbolic alleles, `*`, `.` and breakends fail on
// their first odd letter)
bool plain_allele(const std::string& a)
{
	if (a.empty() || a.size() > (size_t)FASIM_MAX_ALLELE) return false;
	for (char c : a) if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N')) return false;
	return true;
}

// one GT allele: `.` (-1) or an index of the line's alleles
bool gt_allele(const std::string& a, int64_t nalt, int64_t& x)
{
	if (a == ".") { x = -1; return true; }
	for (char c : a) if (!isdigit((unsigned char)c)) return false;
	return parse_int(a, x) && x <= nalt;
}

// fasim_read_vcf; with `sample` the genotypes of that sample as well (fasim_read_vcf_sample)
int read_vcf_impl(const char* path, const char* sample, fasim_variant** out, int64_t* n, fasim_genotype** gts)
{
	if (!path || !out || !n || (sample && !gts)) return fail(nullptr, FASIM_E_ARG, "bad arguments");
	*out = nullptr; *n = 0;
	if (gts) *gts = nullptr;
	std::ifstream in(path);
	if (!in) return fail(nullptr, FASIM_E_ARG, "cannot read VCF file %s", path);
	std::vector<VcfRow> rows;
	std::vector<fasim_genotype> calls;
	std::string line;
	int64_t ln = 0;
	size_t strbytes = 0;
	int64_t sample_col = -1;            // column of the sample (>= 9) once the #CHROM line was read
	while (std::getline(in, line)) {
		ln++;
		while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
		if (sample && line.compare(0, 6, "#CHROM") == 0) {
			int64_t col = 0;
			for (size_t b = 0; ; col++) {
				const size_t e = line.find('\t', b);
				if (col >= 9 && line.compare(b, e == std::string::npos ? std::string::npos : e - b, sample) == 0) { sample_col = col; break; }
				if (e == std::string::npos) break;
				b = e + 1;
			}
			if (sample_col < 0) return fail(nullptr, FASIM_E_ARG, "%s line %lld: the #CHROM line names no sample '%s'", path, (long long)ln, sample);
			continue;
		}
		if (line.empty() || line[0] == '#' || line.find_first_not_of(" \t") == std::string::npos) continue;
		if (sample && sample_col < 0) return fail(nullptr, FASIM_E_ARG, "%s line %lld: no #CHROM line before the first data line: sample '%s' is unknown", path, (long long)ln, sample);
		const size_t want = sample ? (size_t)sample_col + 1 : 5;
		std::vector<std::string> f;
		for (size_t b = 0; f.size() < want; ) {
			const size_t e = line.find('\t', b);
			f.emplace_back(line, b, e == std::string::npos ? std::string::npos : e - b);
			if (e == std::string::npos) break;
			b = e + 1;
		}
		if (f.size() < 5) return fail(nullptr, FASIM_E_ARG, "%s line %lld: fewer than 5 columns", path, (long long)ln);
		int64_t pos = 0;
		if (!parse_int(f[1], pos)) return fail(nullptr, FASIM_E_ARG, "%s line %lld: POS '%s' is not an integer", path, (long long)ln, f[1].c_str());
		if (pos < 1) return fail(nullptr, FASIM_E_ARG, "%s line %lld: POS %lld < 1", path, (long long)ln, (long long)pos);
		if (f[3].empty()) return fail(nullptr, FASIM_E_ARG, "%s line %lld: empty REF", path, (long long)ln);
		if (f[4].empty()) return fail(nullptr, FASIM_E_ARG, "%s line %lld: empty ALT", path, (long long)ln);
		for (char& c : f[3]) c = (char)toupper((unsigned char)c);
		for (char& c : f[4]) c = (char)toupper((unsigned char)c);
		// the call of the sample on this line: up to two alleles, each `.` or an index of the line's alleles
		int64_t call[2] = { -1, -1 }; bool phased = false;
		if (sample) {
			if (f.size() < want) return fail(nullptr, FASIM_E_ARG, "%s line %lld: no column of sample '%s' (%zu columns)", path, (long long)ln, sample, f.size());
			int64_t gi = -1, k = 0;
			for (size_t b = 0; ; k++) {
				const size_t e = f[8].find(':', b);
				if (f[8].compare(b, e == std::string::npos ? std::string::npos : e - b, "GT") == 0) { gi = k; break; }
				if (e == std::string::npos) break;
				b = e + 1;
			}
			if (gi < 0) return fail(nullptr, FASIM_E_ARG, "%s line %lld: no GT in FORMAT '%s'", path, (long long)ln, f[8].c_str());
			const std::string& col = f[(size_t)sample_col];
			size_t b = 0;
			for (k = 0; k < gi && b != std::string::npos; k++) { b = col.find(':', b); if (b != std::string::npos) b++; }
			const std::string gt = b == std::string::npos ? std::string() : col.substr(b, col.find(':', b) == std::string::npos ? std::string::npos : col.find(':', b) - b);
			const int64_t nalt = (int64_t)std::count(f[4].begin(), f[4].end(), ',') + 1;
			const size_t sep = gt.find_first_of("|/");
			bool ok = !gt.empty();
			if (ok && sep == std::string::npos) { ok = gt_allele(gt, nalt, call[0]); call[1] = call[0]; phased = true; }      // haploid
			else if (ok) { ok = gt_allele(gt.substr(0, sep), nalt, call[0]) && gt_allele(gt.substr(sep + 1), nalt, call[1]); phased = gt[sep] == '|'; }
			if (!ok) return fail(nullptr, FASIM_E_ARG, "%s line %lld: malformed GT '%s' of sample '%s'", path, (long long)ln, gt.c_str(), sample);
		}
		const int64_t first_call = (int64_t)calls.size();
		for (size_t b = 0; ; ) {
			const size_t e = f[4].find(',', b);
			VcfRow r;
			r.line = ln; r.pos = pos - 1; r.chrom = f[0]; r.id = f[2]; r.ref = f[3];
			r.alt = f[4].substr(b, e == std::string::npos ? std::string::npos : e - b);
			if (r.alt.empty()) return fail(nullptr, FASIM_E_ARG, "%s line %lld: empty ALT", path, (long long)ln);
			r.usable = plain_allele(r.ref) && plain_allele(r.alt);
			strbytes += r.chrom.size() + r.id.size() + r.ref.size() + r.alt.size() + 4;
			rows.push_back(std::move(r));
			if (sample) {
				const int64_t a = (int64_t)calls.size() - first_call + 1;      // this ALT's index on its line
				fasim_genotype g;
				for (int h = 0; h < 2; h++) g.hap[h] = (int8_t)(call[h] < 0 ? -1 : call[h] == a ? 1 : 0);
				g.phased = phased ? 1 : 0; g.pad = 0;
				calls.push_back(g);
			}
			if (e == std::string::npos) break;
			b = e + 1;
		}
	}
	const size_t head = rows.size() * sizeof(fasim_variant);
	char* block = (char*)malloc(head + strbytes + 1);
	if (!block) return fail(nullptr, FASIM_E_NOMEM, "out of host memory for %zu variants", rows.size());
	fasim_variant* v = (fasim_variant*)block;
	char* s = block + head;
	auto put = [&s](const std::string& x) { const char* at = s; memcpy(s, x.c_str(), x.size() + 1); s += x.size() + 1; return at; };
	for (size_t k = 0; k < rows.size(); k++) {
		const VcfRow& r = rows[k];
		v[k].line = r.line; v[k].pos = r.pos; v[k].rec = 0;
		v[k].ref_len = (int32_t)std::min<size_t>(r.ref.size(), 0x7fffffff); v[k].alt_len = r.usable ? (int32_t)r.alt.size() : -1;
		v[k].chrom = put(r.chrom); v[k].id = put(r.id); v[k].ref = put(r.ref); v[k].alt = put(r.alt);
	}
	if (sample) {
		fasim_genotype* g = (fasim_genotype*)malloc((calls.size() + 1) * sizeof(fasim_genotype));
		if (!g) { free(block); return fail(nullptr, FASIM_E_NOMEM, "out of host memory for %zu genotypes", calls.size()); }
		if (!calls.empty()) memcpy(g, calls.data(), calls.size() * sizeof(fasim_genotype));
		*gts = g;
	}
	*out = v; *n = (int64_t)rows.size();
	return FASIM_OK;
}

}  // namespace

int fasim_read_vcf(const char* path, fasim_variant** out, int64_t* n) { return read_vcf_impl(path, nullptr, out, n, nullptr); }

int fasim_read_vcf_sample(const char* path, const char* sample, fasim_variant** out, int64_t* n, fasim_genotype** gts)
{
	if (!sample || !*sample) return fail(nullptr, FASIM_E_ARG, "no sample name given");
	return read_vcf_impl(path, sample, out, n, gts);
}
