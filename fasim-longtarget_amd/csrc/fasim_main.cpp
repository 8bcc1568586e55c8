// fasim -- CLI driver with the reference's flags (initEnv(), Fasim-LongTarget.cpp:269-377) and output files
// (printResult(), :797-829), calling the HIP path through the C-ABI of libfasim_hip.so.
//
//   fasim -f1 DNA.fa -f2 RNA.fa [-r R] [-O outdir] [-c cut] [-o overlap] [-t strand] [-i identity]
//         [-S stability] [-ni ntmin] [-na ntmax] [-pc C] [-pt T] [-ds dist] [-lg len] [-cn n]
//   extras (none of them changes what is computed for an input the reference handles):
//     --device N            HIP device (default 0)
//     --devices LIST        several devices of one node, e.g. 0-7 or 0,1,2: the segments of every DNA record are cut
//                           into contiguous shards, one engine (host thread) per device, records merged in shard order
//     --all-records         scan EVERY record of a multi-record DNA file (a genome), one record in memory at a time, and
//                           write one set of output files per record: <species>-<lnc>-<f1 stem>.<chr>-TFOsorted / -TFOclass...
//                           Consecutive short records (peaks, promoter windows) are scanned in groups of about
//                           FASIM_RECORD_GROUP segments (default 5120) by one fasim_scan_records call each; a record of that
//                           many segments or more is scanned alone; FASIM_RECORD_GROUP=0 scans every record alone
//     --regions FILE.bed    scan the BED intervals of a genome (fasim_read_bed): every interval gets the files --all-records
//                           writes for the record >NAME|CHROM|START+1-END of its bytes, plus one index per lncRNA,
//                           <O>/<lnc>-<f1 stem>.regions.tsv; the genome is streamed and the intervals are grouped as above.
//                           Exit status 2 for a refused BED file (nothing written), 1 if an interval lies in no DNA record
//     --accumulate-records  bug-compatible with the reference's reader (defect B1, Fasim-LongTarget.cpp:219-262): record
//                           k is scanned as the concatenation of records 1..k, later headers are parsed with the stale
//                           field counter, everything is written into ONE output set named after the first record
//     --track BIN           per-base triplex potential (fasim_scan_track): a fourth file <stem>-TFOpotential-<BIN> per lncRNA and
//                           record, a bedGraph with one block per strand class and one value per BIN bases (the best local
//                           alignment score that ends there, no candidate threshold); --track-min V leaves out bins below V
//                           (default 1); --track-only writes only that file and skips stage 3.  With --all-records the records are
//                           grouped as above (fasim_scan_records_track).  Not with --regions, --accumulate-records or -F (exit status 2)
//     --tfo-profile         per-base profile of the lncRNA (fasim_scan_tfo_profile): per strand class and base of
//                           the lncRNA the best local alignment score that ends on that base.  A plain run writes a fourth file
//                           <stem>-TFOprofile per lncRNA; with --all-records or --regions one whole-set table per lncRNA,
//                           <O>/<lnc>-<f1 stem>.tfoprofile.tsv.  --tfo-profile-only writes only the table and runs no stage 3.
//                           Not with -F, --accumulate-records, --track or --screen (exit status 2, nothing written)
//     --sites V             sites above a fixed potential (fasim_scan_records_sites): the ranges of positions whose
//                           potential in one strand class reaches V (1 .. 16 383), ranges at most --sites-gap G (default 0) apart joined,
//                           as BED lines chrom start end class value strand peak rule.  A plain run writes <stem>-TFOsites-<V> next to
//                           -TFOsorted; with --all-records or --regions one file per lncRNA, <O>/<lnc>-<f1 stem>.sites-<V>.bed, the
//                           records' sites in record / BED order with the record's name as a ninth column.  --sites-only writes nothing
//                           else and runs no stage 3.  Exit status 2, nothing written: V outside [1, 16383], a negative G, --sites-gap or
//                           --sites-only without --sites, --sites with -F, --accumulate-records, --track, --screen or --tfo-profile
//     --oligos              with --sites V: every record of -f2 is one short oligo of 1 .. 112 nt and the run is a panel scan
//                           (fasim_scan_oligos): per oligo the sites file that --sites V --sites-only writes for a
//                           lncRNA of that name, and one panel table <O>/<f2 stem>-<f1 stem>.oligos-<V>.tsv (per oligo: sites, covered bases,
//                           per class sites and largest value).  Never -TFOsorted / -TFOclass.  Exit status 2, nothing written: without
//                           --sites (or --potential-hist, --oligo-profile, --oligo-screen), with --sites-align, -F, --track, --screen, --tfo-profile or --accumulate-records, or an -f2
//                           record that is empty or longer than 112 nt
//     --oligo-hits          with --oligos --sites V: every site of every oligo with its hit (fasim_scan_oligos_aligned, DESIGN.md section
//                           18): beside each oligo's sites file the table that --sites V --sites-only --sites-align writes for a lncRNA
//                           of that name (<stem>-TFOsites-<V>-aligned; set mode <O>/<oligo>-<f1 stem>.sites-<V>.aligned.tsv).  The sites
//                           files and the panel table are what they are without it.  Exit status 2, nothing written: without --oligos,
//                           without --sites, with --potential-hist
//     --oligo-profile       with --oligos: the per-base profile of every oligo (fasim_scan_oligos_profile), the table
//                           --tfo-profile writes for a lncRNA of that name: a plain run <stem>-TFOprofile (the stem of the oligo's
//                           -TFOsites-<V> file), with --all-records or --regions one whole-set table <O>/<oligo>-<f1 stem>.tfoprofile.tsv
//     --oligo-screen        with --oligos and --all-records or --regions: the screen of every oligo (fasim_scan_oligos_peaks),
//                           <O>/<oligo>-<f1 stem>.screen.tsv, the table --screen-only writes for a lncRNA of that name.  --oligos is
//                           satisfied by --sites V, --potential-hist, --oligo-profile or --oligo-screen; the two may be given together
//                           and with --sites V [--sites-gap G], whose files are then what they are without them.  Exit status 2, nothing
//                           written: either without --oligos, --oligo-screen without --all-records / --regions, either with
//                           --potential-hist or --oligo-hits
//     --potential-hist      histogram of the potential with shuffled controls (fasim_scan_records_hist): per
//                           strand class and value how many bases of the DNA reach it.  --hist-controls K (default 0) scans K
//                           composition-preserving shuffles of every lncRNA too (--hist-seed S, default 0) and reports the false discovery
//                           rate per value and the smallest value that keeps it at or below --hist-fdr Q (default 0.05) as min_value, a
//                           defensible V for --sites.  A plain run writes <stem>-TFOhist next to -TFOsorted; with --all-records or
//                           --regions one table per lncRNA over the whole set, <O>/<lnc>-<f1 stem>.hist.tsv; with --oligos one such table
//                           per oligo and nothing else.  --potential-hist-only writes nothing else and runs no stage 3.  Exit status 2,
//                           nothing written: with -F, --accumulate-records, --track, --screen, --tfo-profile or --sites, --hist-* or
//                           --potential-hist-only without --potential-hist, K < 0, Q outside (0, 1], -o above half of -c
//     --hist-sites          with --potential-hist: the sites per threshold too (fasim_scan_records_site_counts).
//                           Beside the unchanged hist table <stem>-TFOsitecounts (set mode <O>/<lnc>-<f1 stem>.sitecounts.tsv, with
//                           --oligos one per oligo): per value the number of sites --sites V --sites-gap 0 would report, per class,
//                           with the controls' and the false discovery rate per site.  --hist-shuffle mono|di (default mono) draws
//                           the controls of both tables with fasim_shuffle_query or, keeping the dinucleotide counts, with
//                           fasim_shuffle_query_dinuc.  Exit status 2, nothing written: either without --potential-hist, a value
//                           other than mono / di
//     --sites-align         with --sites V: every site with its hit (fasim_scan_records_sites_aligned), the local
//                           alignment behind the site's peak: beside the sites file <stem>-TFOsites-<V>-aligned (set mode:
//                           <O>/<lnc>-<f1 stem>.sites-<V>.aligned.tsv, the record's name as a last column), a `# fasim site hits` line,
//                           a header line, then one line per site in the order of the sites file: chrom tts_start tts_end class value
//                           strand rule tfo_start tfo_end nt identity stability cigar TFO TTS.  Without --sites: status 2
//     --variants FILE.vcf   every (VCF line, ALT allele) scored by the triplex potential through it, for REF and for ALT, within
//                           --variant-flank F (default 300, at most 2048) bases: one table per lncRNA,
//                           <O>/<lnc>-<f1 minus 3 chars>.variants.tsv, and nothing else (fasim_score_variants).
//                           Exit status 2, nothing written: a malformed VCF, --variant-flank outside [0, 2048] or without
//                           --variants, --variants with --regions, --all-records, --accumulate-records, -F, --track, --screen,
//                           --tfo-profile, --sites, --oligos, --potential-hist or --devices
//     --variant-hits        with --variants: the alignment behind every score as well, a second table per lncRNA,
//                           <O>/<lnc>-<f1 minus 3 chars>.variants.hits.tsv (fasim_score_variants_aligned): a
//                           header line, then one line per (VCF line, ALT, allele, class) with a value: line chrom pos id ref alt
//                           allele class value rule strand tts_start tts_end tfo_start tfo_end nt identity stability cigar clipped
//                           TFO TTS.  The .variants.tsv file does not change.  Without --variants: status 2
//     --sample NAME         with --variants: every entry scored on the two haplotypes of sample NAME of the VCF as well (GT through
//                           FORMAT, the sample by its name in the #CHROM line): the haplotype's other variants, where they are
//                           phased or homozygous, stand in the window.  One more table per lncRNA,
//                           <O>/<lnc>-<f1 minus 3 chars>.haplotypes.tsv (fasim_score_haplotypes); the other
//                           tables do not change.  Status 2, nothing written: without --variants, a sample the VCF does not name,
//                           a line without its column, no GT in FORMAT, a malformed GT
//     --mutagenesis FILE.bed  every substitution at every position of the BED intervals, scored by the triplex potential through it
//                           from one shared pass per interval (fasim_score_mutagenesis): per lncRNA one table,
//                           <O>/<lnc>-<f1 minus 3 chars>.mutagenesis.tsv, and nothing else; --mutagenesis-flank F (default 300, 0 to
//                           2048) is the context on either side of an interval, which may have 5120 - 2 F positions.  Status 2,
//                           nothing written: a bad BED file, an interval too long, a flank out of range or without --mutagenesis,
//                           --mutagenesis with --variants, --regions, --all-records, --accumulate-records, -F, --track, --screen,
//                           --tfo-profile, --sites, --oligos, --potential-hist or --devices
//     --deletions LIST      with --mutagenesis: every deletion of d bases, d of LIST (1 to 16 strictly ascending integers in
//                           1 ... 1023, comma-separated), behind every position of the intervals and inside them, from a shared
//                           pass of its own (fasim_score_deletions): one more table per lncRNA, <O>/<lnc>-<f1 minus 3
//                           chars>.deletions.tsv; the mutagenesis table does not change.  --deletions-only writes only the new table
//                           and runs no SNV problems.  Status 2, nothing written: either without --mutagenesis, --deletions-only
//                           without --deletions, a list that is empty, not ascending, not integers, out of range or too long
//     --screen              with --regions or --all-records: one table per lncRNA, <O>/<lnc>-<f1 stem>.screen.tsv, one line per
//                           interval (BED order) or record: per strand class the peak of its potential, where it lies (0-based
//                           genome coordinate) and the rule of the encoding that attains it (fasim_screen_tsv, DESIGN.md section
//                           12).  --screen-only writes nothing else and runs no stage 3.  Exit status 2, nothing written: --screen
//                           without --regions / --all-records, with --accumulate-records or -F, --screen-only with --track
//     --upper               upper-case the DNA while reading (soft-masked genomes; the reference treats lower case as N)
//     --clamp-cluster       defined behaviour where the reference's clustering does not terminate (see fasim_hip.h)
//     --stats               timing/statistics on stderr (parse, scan, tail, write)
//   -f2 may hold several lncRNAs (one '>' record each): every lncRNA is scanned against the DNA record while it is
//   resident (fasim_scan_queries) and gets its own output set.  A single-record -f2 behaves exactly like the reference.
//
// Differences, all documented in DESIGN.md: without --all-records / --accumulate-records only the first record of a
// multi-record DNA file is scanned; -d is parsed and ignored as in the reference.  -F (classic SIM): the forward sweep runs
// on the GPU, the rest of SIM() on host threads (first version of that path).
#include <getopt.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fasim_hip.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DnaRecord { std::string header, species, chr, seq; long start = 0; };

static void strip_eol(std::string& s) { s.erase(std::remove(s.begin(), s.end(), '\r'), s.end()); s.erase(std::remove(s.begin(), s.end(), '\n'), s.end()); }

// header '>species|chr|start-end' as readDna() parses it (Fasim-LongTarget.cpp:226-255).  `field` is the reference's
// counter j: it is never reset there, so in --accumulate-records mode it is carried from header to header and the
// second and later headers keep the first record's species / chr and get atoi("species|chr|start") as their start.
struct HeaderParser {
	int field = 0;
	std::string species, chr, start;
	void parse(const std::string& line)
	{
		std::string tmp;
		for (char c : line) {
			if (c == '>') { tmp.clear(); continue; }
			if (c == '|' && field == 0) { species = tmp; field++; tmp.clear(); continue; }
			if (c == '|' && field == 1) { chr = tmp; field++; tmp.clear(); continue; }
			if (c == '-' && field == 2) { start = tmp; tmp.clear(); continue; }
			tmp += c;
		}
	}
};

// streaming FASTA reader: one record at a time (a genome never sits in memory as a whole)
struct DnaReader {
	std::ifstream in; std::string pending; bool have_pending = false; bool upper = false; bool sticky_fields = false;
	HeaderParser hp;
	bool open(const std::string& path) { in.open(path); return (bool)in; }
	bool next(DnaRecord& r)
	{
		std::string line;
		if (!have_pending) {
			while (std::getline(in, line)) if (!line.empty() && line[0] == '>') { pending = line; have_pending = true; break; }
			if (!have_pending) return false;
		}
		r = DnaRecord();
		if (!sticky_fields) hp = HeaderParser();
		hp.parse(pending);
		r.header = pending;
		r.species = hp.species; r.chr = hp.chr; r.start = atoi(hp.start.c_str());
		have_pending = false;
		while (std::getline(in, line)) {
			if (!line.empty() && line[0] == '>') { pending = line; have_pending = true; break; }
			strip_eol(line); r.seq += line;
		}
		if (upper) fasim_upper_case(&r.seq[0], (int64_t)r.seq.size());
		return true;
	}
};

struct Rna { std::string name, seq; };

// One '>' record: exactly readRna() (Fasim-LongTarget.cpp:174-200): the name is the first line without '>' characters.
// Several records: one lncRNA each (the reference would glue the later header lines into the sequence).
static bool read_rnas(const std::string& path, std::vector<Rna>& out)
{
	std::ifstream in(path);
	if (!in) return false;
	std::string line;
	bool first = true;
	while (std::getline(in, line)) {
		if (first || (!line.empty() && line[0] == '>')) {
			Rna r;
			for (char c : line) if (c != '>') r.name += c;
			strip_eol(r.name);
			out.push_back(r);
			first = false;
			continue;
		}
		strip_eol(line); out.back().seq += line;
	}
	return !out.empty();
}

// the whole of `s` as a decimal int; `bad` (a value the caller refuses) where it is empty, has trailing characters or does not fit
static int strict_int(const char* s, int bad)
{
	char* end = nullptr;
	errno = 0;
	const long v = strtol(s, &end, 10);
	if (end == s || *end != '\0' || errno == ERANGE || v < -2147483647L - 1 || v > 2147483647L) return bad;
	return (int)v;
}

// "0-7", "0,1,2", "0,0,0"
static std::vector<int> parse_devices(const char* s)
{
	std::vector<int> v;
	const char* p = s;
	while (*p) {
		char* e = nullptr;
		const long a = strtol(p, &e, 10);
		if (e == p) break;
		long b = a;
		p = e;
		if (*p == '-') { b = strtol(p + 1, &e, 10); p = e; }
		for (long k = a; k <= b; k++) v.push_back((int)k);
		if (*p == ',') p++;
	}
	return v;
}

// returns 0 when every byte reached the file (a missing -O directory or a full disk must not end in "finished normally")
static int write_file(const std::string& path, const char* text, int64_t len)
{
	std::ofstream of(path.c_str(), std::ios::trunc);
	if (of) of.write(text, (std::streamsize)len);
	of.close();
	if (!of) { fprintf(stderr, "fasim: cannot write %s\n", path.c_str()); return 1; }
	return 0;
}

struct Timers { double parse = 0, scan = 0, tail = 0, write = 0, tail_wait = 0; };

// -TFOsorted + the two -TFOclass files of one lncRNA (printResult(), Fasim-LongTarget.cpp:797-836): one clustering, three texts
// (*data_lines, if given: the lines of -TFOsorted after its header line)
static int write_outputs(const fasim_result* res, const std::string& stem, const std::string& chr, long start, int64_t dna_len,
	const std::string& lnc_name, const fasim_params& p, int flags, Timers& tm, int64_t* data_lines = nullptr)
{
	char* text[3] = { nullptr, nullptr, nullptr }; int64_t len[3] = { 0, 0, 0 };
	double t0 = now_s();
	if (fasim_tail_outputs(res->recs, res->count, res->pool, res->pool_len, chr.c_str(), start, dna_len, lnc_name.c_str(), &p, flags,
		&text[0], &len[0], &text[1], &len[1], &text[2], &len[2]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
	tm.tail += now_s() - t0; t0 = now_s();
	if (data_lines) *data_lines = std::max<int64_t>(0, (int64_t)std::count(text[0], text[0] + len[0], '\n') - 1);
	int bad = write_file(stem + "-TFOsorted", text[0], len[0]);
	for (int level = 1; level <= 2; level++)     // print_cluster x2 (:832-836): <prefix>-TFOclass<level>-<ds>-<lg> (:706)
		bad |= write_file(stem + "-TFOclass" + std::to_string(level) + "-" + std::to_string(p.cDistance) + "-" + std::to_string(p.cLength), text[level], len[level]);
	for (char* t : text) fasim_free(t);
	tm.write += now_s() - t0;
	return bad;
}

// The host tail of record i (clustering, text, file writes) runs on its own thread while the devices already scan record
// i+1; at most `kMaxPending` results wait to be written.
static std::mutex g_out_mu;
static int g_out_failed = 0;

// --track: bin width (0: no tracks), smallest value written, --track-only; --screen / --screen-only: peaks (no_stage3: no records)
// --tfo-profile / --tfo-profile-only: the lncRNA's profile (never together with tracks or peaks)
// --sites V / --sites-gap G / --sites-only: the sites above a fixed potential (never together with tracks, peaks or the profile)
struct TrackOpt { int bin = 0, min_value = 1; bool only = false, peaks = false, no_stage3 = false, tfo = false, tfo_only = false; int sites = 0, sites_gap = 0; bool sites_only = false, sites_align = false, oligos = false, oligo_hits = false, oligo_profile = false, oligo_screen = false;
	bool hits() const { return sites_align || oligo_hits; }      // the sites' hits are wanted (--sites-align, or --oligo-hits of a panel)
	// --potential-hist: the histogram, K controls per lncRNA under a seed (hist_ctl: their sequences, lncRNA after lncRNA), the FDR bound
	bool hist = false, hist_only = false; int hist_controls = 0; uint64_t hist_seed = 0; double hist_fdr = 0.05; const std::vector<std::string>* hist_ctl = nullptr;
	// --hist-sites: site counts in the place of the histograms (their n[][] is the histogram); --hist-shuffle di: dinucleotide controls
	bool hist_sites = false, hist_dinuc = false; };

// acc += part by fasim_hist_merge (different groups of records: nothing pairs); takes `part` over
static int hist_fold(fasim_hist*& acc, fasim_hist* part)
{
	if (!acc) { acc = part; return 0; }
	const fasim_hist* two[2] = { acc, part };
	fasim_hist* sum = nullptr;
	const int rc = fasim_hist_merge(two, 2, &sum);
	fasim_hist_free(part);
	if (rc != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
	fasim_hist_free(acc);
	acc = sum;
	return 0;
}

// the same for site counts (--hist-sites)
static int counts_fold(fasim_site_counts*& acc, fasim_site_counts* part)
{
	if (!acc) { acc = part; return 0; }
	const fasim_site_counts* two[2] = { acc, part };
	fasim_site_counts* sum = nullptr;
	const int rc = fasim_site_counts_merge(two, 2, &sum);
	fasim_site_counts_free(part);
	if (rc != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
	fasim_site_counts_free(acc);
	acc = sum;
	return 0;
}

// acc = max(acc, part) by fasim_tfo_profile_merge; takes `part` over
static int tfo_fold(fasim_tfo_profile*& acc, fasim_tfo_profile* part)
{
	if (!acc) { acc = part; return 0; }
	const fasim_tfo_profile* two[2] = { acc, part };
	fasim_tfo_profile* sum = nullptr;
	const int rc = fasim_tfo_profile_merge(two, 2, &sum);
	fasim_tfo_profile_free(part);
	if (rc != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
	fasim_tfo_profile_free(acc);
	acc = sum;
	return 0;
}

// Scans one DNA record with every lncRNA on every device: device d takes the d-th contiguous block of segments
// (SURVEY 8(e)); per lncRNA the shard results are merged in shard order, which is the reference's canonical order.
// With --track the potential tracks come back in `tracks` (shards merged by maximum); --track-only leaves `out` NULL.
static int scan_record(const std::vector<fasim_engine*>& engines, const std::vector<Rna>& rnas, const char* dna, int64_t dna_len, const fasim_params& p,
	std::vector<fasim_result*>& out, const TrackOpt& trk, std::vector<fasim_track*>& tracks, std::vector<fasim_tfo_profile*>* profs = nullptr)
{
	const int nd = (int)engines.size(), nq = (int)rnas.size();
	const bool no_res = trk.only || trk.tfo_only;
	if (profs) profs->assign((size_t)nq, nullptr);
	std::vector<const char*> qp((size_t)nq); std::vector<int32_t> ql((size_t)nq);
	for (int q = 0; q < nq; q++) { qp[(size_t)q] = rnas[(size_t)q].seq.data(); ql[(size_t)q] = (int32_t)rnas[(size_t)q].seq.size(); }
	out.assign((size_t)nq, nullptr);
	tracks.assign(trk.bin ? (size_t)nq : 0, nullptr);
	auto scan = [&](fasim_engine* e, int64_t first, int64_t count, fasim_result** res, fasim_track** tr, fasim_tfo_profile** pf) {
		// (--tfo-profile: the record as a set of one; its records are those of fasim_scan_queries)
		const int64_t off0 = 0;
		if (profs) return fasim_scan_tfo_profile(e, qp.data(), ql.data(), nq, dna, &off0, &dna_len, 1, first, count, &p, 0, no_res ? nullptr : res, pf, nullptr);
		if (!trk.bin) return fasim_scan_queries(e, qp.data(), ql.data(), nq, dna, dna_len, first, count, &p, res);
		return fasim_scan_track(e, qp.data(), ql.data(), nq, dna, dna_len, first, count, &p, trk.bin, trk.only ? nullptr : res, tr);
	};
	if (nd == 1) {
		if (scan(engines[0], 0, -1, out.data(), tracks.data(), profs ? profs->data() : nullptr) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(engines[0])); return 1; }
		return 0;
	}
	const int64_t nseg = fasim_segment_count(dna_len, &p);
	std::vector<std::vector<fasim_result*>> part((size_t)nd, std::vector<fasim_result*>((size_t)nq, nullptr));
	std::vector<std::vector<fasim_track*>> tpart((size_t)nd, std::vector<fasim_track*>((size_t)nq, nullptr));
	std::vector<std::vector<fasim_tfo_profile*>> fpart((size_t)nd, std::vector<fasim_tfo_profile*>((size_t)nq, nullptr));
	std::vector<int> rc((size_t)nd, 0);
	std::vector<std::thread> th;
	for (int d = 0; d < nd; d++) {
		th.emplace_back([&, d] {
			const int64_t base = nseg / nd, rem = nseg % nd;
			const int64_t first = d * base + std::min<int64_t>(d, rem), count = base + (d < rem ? 1 : 0);
			rc[(size_t)d] = scan(engines[(size_t)d], first, count, part[(size_t)d].data(), tpart[(size_t)d].data(), fpart[(size_t)d].data());
		});
	}
	for (auto& t : th) t.join();
	int bad = 0;
	for (int d = 0; d < nd; d++) if (rc[(size_t)d] != FASIM_OK) { fprintf(stderr, "fasim: device shard %d: %s\n", d, fasim_last_error(engines[(size_t)d])); bad = 1; }
	for (int q = 0; q < nq && !bad && trk.bin; q++) {
		std::vector<const fasim_track*> tp((size_t)nd);
		for (int d = 0; d < nd; d++) tp[(size_t)d] = tpart[(size_t)d][(size_t)q];
		if (fasim_track_merge(tp.data(), nd, &tracks[(size_t)q]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (auto& v : tpart) for (fasim_track* t : v) fasim_track_free(t);
	for (int q = 0; q < nq && !bad && profs; q++) {
		std::vector<const fasim_tfo_profile*> fp((size_t)nd);
		for (int d = 0; d < nd; d++) fp[(size_t)d] = fpart[(size_t)d][(size_t)q];
		if (fasim_tfo_profile_merge(fp.data(), nd, &(*profs)[(size_t)q]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (auto& v : fpart) for (fasim_tfo_profile* t : v) fasim_tfo_profile_free(t);
	for (int q = 0; q < nq && !bad && !no_res; q++) {
		std::vector<const fasim_triplex*> recs((size_t)nd); std::vector<int64_t> counts((size_t)nd), plens((size_t)nd); std::vector<const char*> pools((size_t)nd);
		for (int d = 0; d < nd; d++) { const fasim_result* r = part[(size_t)d][(size_t)q]; recs[(size_t)d] = r->recs; counts[(size_t)d] = r->count; pools[(size_t)d] = r->pool; plens[(size_t)d] = r->pool_len; }
		if (fasim_merge_results(recs.data(), counts.data(), pools.data(), plens.data(), nd, &out[(size_t)q]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; break; }
		// statistics of the merged result: sums over the shards (times: the slowest shard)
		fasim_scan_stats& st = out[(size_t)q]->stats;
		for (int d = 0; d < nd; d++) {
			const fasim_scan_stats& x = part[(size_t)d][(size_t)q]->stats;
			st.segments += x.segments; st.segments_skipped += x.segments_skipped; st.units += x.units; st.candidates += x.candidates;
			st.align_calls += x.align_calls; st.logical_cells += x.logical_cells; st.hazard_units += x.hazard_units;
			st.t_total_s = std::max(st.t_total_s, x.t_total_s);
		}
	}
	for (auto& v : part) for (fasim_result* r : v) fasim_result_free(r);
	if (bad) { for (fasim_track*& t : tracks) { fasim_track_free(t); t = nullptr; } }
	if (bad && profs) for (fasim_tfo_profile*& t : *profs) { fasim_tfo_profile_free(t); t = nullptr; }
	return bad;
}

// --all-records / --regions: consecutive short records scanned together, one fasim_scan_records call per group (all lncRNAs, all
// devices); record r of the group is dna[off[r] .. off[r] + len[r]).  out[q][r] = the records of lncRNA q in record r of the
// group, exactly what scan_record gives for that record alone.  With several devices, device d takes the d-th contiguous block of
// the group's global segment list and every record's parts are merged in device order.
static int scan_group(const std::vector<fasim_engine*>& engines, const std::vector<Rna>& rnas, const std::string& dna,
	const std::vector<int64_t>& off, const std::vector<int64_t>& len, const fasim_params& p, std::vector<std::vector<fasim_result*>>& out,
	const TrackOpt& trk, std::vector<std::vector<fasim_track*>>& tracks, std::vector<fasim_peak>& peaks, std::vector<fasim_tfo_profile*>* profs = nullptr,
	std::vector<std::vector<fasim_sites*>>* sites = nullptr, std::vector<std::vector<fasim_site_hits*>>* hits = nullptr,
	std::vector<fasim_hist*>* hists = nullptr, std::vector<fasim_site_counts*>* counts = nullptr)
{
	const int nd = (int)engines.size(), nq = (int)rnas.size(), nrec = (int)off.size();
	// --potential-hist: one histogram per lncRNA over the group, then those of its controls ([nq] + [nq * K], as hist_ctl)
	// (--hist-sites: `counts` in the place of `hists`, the same queries)
	const int nctl = (hists || counts) && trk.hist_ctl ? (int)trk.hist_ctl->size() : 0;
	std::vector<const char*> hq; std::vector<int32_t> hl;
	if (hists || counts) {
		for (int q = 0; q < nq; q++) { hq.push_back(rnas[(size_t)q].seq.data()); hl.push_back((int32_t)rnas[(size_t)q].seq.size()); }
		for (int k = 0; k < nctl; k++) { hq.push_back((*trk.hist_ctl)[(size_t)k].data()); hl.push_back((int32_t)(*trk.hist_ctl)[(size_t)k].size()); }
		if (hists) hists->assign((size_t)(nq + nctl), nullptr);
		if (counts) counts->assign((size_t)(nq + nctl), nullptr);
	}
	std::vector<std::vector<fasim_site_counts*>> cpart((size_t)nd, std::vector<fasim_site_counts*>(counts ? (size_t)(nq + nctl) : 0, nullptr));
	std::vector<std::vector<fasim_hist*>> gpart((size_t)nd, std::vector<fasim_hist*>(hists ? (size_t)(nq + nctl) : 0, nullptr));
	std::vector<const char*> qp((size_t)nq); std::vector<int32_t> ql((size_t)nq);
	for (int q = 0; q < nq; q++) { qp[(size_t)q] = rnas[(size_t)q].seq.data(); ql[(size_t)q] = (int32_t)rnas[(size_t)q].seq.size(); }
	int64_t nseg = 0;
	for (int r = 0; r < nrec; r++) nseg += fasim_segment_count(len[(size_t)r], &p);
	const bool with_track = trk.bin > 0, with_peaks = trk.peaks, no_res = trk.no_stage3;
	const size_t nout = (size_t)nq * nrec;
	out.assign((size_t)nq, std::vector<fasim_result*>((size_t)nrec, nullptr));
	tracks.assign(with_track ? (size_t)nq : 0, std::vector<fasim_track*>((size_t)nrec, nullptr));
	peaks.clear();
	std::vector<std::vector<fasim_result*>> part((size_t)nd, std::vector<fasim_result*>(nout, nullptr));
	std::vector<std::vector<fasim_track*>> tpart((size_t)nd, std::vector<fasim_track*>(with_track ? nout : 0, nullptr));
	std::vector<std::vector<fasim_peak>> ppart((size_t)nd, std::vector<fasim_peak>(with_peaks ? nout * 4 : 0));
	// --tfo-profile: one profile per lncRNA over the whole group
	std::vector<std::vector<fasim_tfo_profile*>> fpart((size_t)nd, std::vector<fasim_tfo_profile*>(profs ? (size_t)nq : 0, nullptr));
	if (profs) profs->assign((size_t)nq, nullptr);
	// --sites: one list per lncRNA and record
	std::vector<std::vector<fasim_sites*>> spart((size_t)nd, std::vector<fasim_sites*>(sites ? nout : 0, nullptr));
	if (sites) sites->assign((size_t)nq, std::vector<fasim_sites*>((size_t)nrec, nullptr));
	// --sites-align: the hits of those sites
	std::vector<std::vector<fasim_site_hits*>> hpart((size_t)nd, std::vector<fasim_site_hits*>(sites && hits ? nout : 0, nullptr));
	if (hits) hits->assign((size_t)nq, std::vector<fasim_site_hits*>((size_t)nrec, nullptr));
	std::vector<int> rc((size_t)nd, 0);
	auto run = [&](int d) {
		const int64_t base = nseg / nd, rem = nseg % nd;
		const int64_t first = d * base + std::min<int64_t>(d, rem), count = base + (d < rem ? 1 : 0);
		if ((trk.oligo_profile || trk.oligo_screen) && !sites) rc[(size_t)d] = FASIM_OK;      // a panel's profiles / peaks alone: their calls below
		else if (counts && trk.oligos)
			rc[(size_t)d] = fasim_scan_oligos_site_counts(engines[(size_t)d], hq.data(), hl.data(), nq + nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				cpart[(size_t)d].data(), nullptr);
		else if (counts && no_res)
			rc[(size_t)d] = fasim_scan_records_site_counts(engines[(size_t)d], hq.data(), hl.data(), nq + nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				nullptr, cpart[(size_t)d].data(), nullptr);
		else if (counts) {
			rc[(size_t)d] = fasim_scan_records_site_counts(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				part[(size_t)d].data(), cpart[(size_t)d].data(), nullptr);
			if (rc[(size_t)d] == FASIM_OK && nctl)
				rc[(size_t)d] = fasim_scan_records_site_counts(engines[(size_t)d], hq.data() + nq, hl.data() + nq, nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
					nullptr, cpart[(size_t)d].data() + nq, nullptr);
		}
		else if (hists && trk.oligos)
			rc[(size_t)d] = fasim_scan_oligos_hist(engines[(size_t)d], hq.data(), hl.data(), nq + nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				gpart[(size_t)d].data(), nullptr);
		else if (hists && no_res)
			rc[(size_t)d] = fasim_scan_records_hist(engines[(size_t)d], hq.data(), hl.data(), nq + nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				nullptr, gpart[(size_t)d].data(), nullptr);
		else if (hists) {
			// stage 3 for the lncRNAs only: their controls go in a histogram-only call of their own
			rc[(size_t)d] = fasim_scan_records_hist(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				part[(size_t)d].data(), gpart[(size_t)d].data(), nullptr);
			if (rc[(size_t)d] == FASIM_OK && nctl)
				rc[(size_t)d] = fasim_scan_records_hist(engines[(size_t)d], hq.data() + nq, hl.data() + nq, nctl, dna.data(), off.data(), len.data(), nrec, first, count, &p,
					nullptr, gpart[(size_t)d].data() + nq, nullptr);
		}
		else if (sites && trk.oligos && hits)
			rc[(size_t)d] = fasim_scan_oligos_aligned(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				trk.sites, trk.sites_gap, spart[(size_t)d].data(), hpart[(size_t)d].data(), nullptr);
		else if (sites && trk.oligos)
			rc[(size_t)d] = fasim_scan_oligos(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				trk.sites, trk.sites_gap, spart[(size_t)d].data(), 0, nullptr, nullptr);
		else if (sites && hits)
			rc[(size_t)d] = fasim_scan_records_sites_aligned(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				trk.sites, trk.sites_gap, no_res ? nullptr : part[(size_t)d].data(), spart[(size_t)d].data(), hpart[(size_t)d].data(), nullptr);
		else if (sites)
			rc[(size_t)d] = fasim_scan_records_sites(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				trk.sites, trk.sites_gap, no_res ? nullptr : part[(size_t)d].data(), spart[(size_t)d].data(), nullptr);
		else if (profs)
			rc[(size_t)d] = fasim_scan_tfo_profile(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p, 0,
				no_res ? nullptr : part[(size_t)d].data(), fpart[(size_t)d].data(), nullptr);
		else if (!with_track && !with_peaks)
			rc[(size_t)d] = fasim_scan_records(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				part[(size_t)d].data(), nullptr);
		else
			rc[(size_t)d] = fasim_scan_records_track(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p,
				trk.bin, no_res ? nullptr : part[(size_t)d].data(), with_track ? tpart[(size_t)d].data() : nullptr,
				with_peaks ? ppart[(size_t)d].data() : nullptr, nullptr);
		// --oligos --oligo-profile / --oligo-screen: one more call per product
		if (rc[(size_t)d] == FASIM_OK && trk.oligo_profile)
			rc[(size_t)d] = fasim_scan_oligos_profile(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p, 0,
				fpart[(size_t)d].data(), nullptr);
		if (rc[(size_t)d] == FASIM_OK && trk.oligo_screen)
			rc[(size_t)d] = fasim_scan_oligos_peaks(engines[(size_t)d], qp.data(), ql.data(), nq, dna.data(), off.data(), len.data(), nrec, first, count, &p, 0,
				nullptr, ppart[(size_t)d].data(), nullptr);
	};
	if (nd == 1) run(0);
	else { std::vector<std::thread> th; for (int d = 0; d < nd; d++) th.emplace_back(run, d); for (auto& t : th) t.join(); }
	int bad = 0;
	for (int d = 0; d < nd; d++) {
		if (rc[(size_t)d] == FASIM_OK) continue;
		if (nd == 1) fprintf(stderr, "fasim: %s\n", fasim_last_error(engines[0]));
		else fprintf(stderr, "fasim: device shard %d: %s\n", d, fasim_last_error(engines[(size_t)d]));
		bad = 1;
	}
	for (int q = 0; q < nq && !bad && !no_res; q++) for (int r = 0; r < nrec && !bad; r++) {
		const size_t k = (size_t)q * nrec + r;
		if (nd == 1) { out[(size_t)q][(size_t)r] = part[0][k]; part[0][k] = nullptr; continue; }
		std::vector<const fasim_triplex*> recs((size_t)nd); std::vector<int64_t> counts((size_t)nd), plens((size_t)nd); std::vector<const char*> pools((size_t)nd);
		for (int d = 0; d < nd; d++) { const fasim_result* x = part[(size_t)d][k]; recs[(size_t)d] = x->recs; counts[(size_t)d] = x->count; pools[(size_t)d] = x->pool; plens[(size_t)d] = x->pool_len; }
		if (fasim_merge_results(recs.data(), counts.data(), pools.data(), plens.data(), nd, &out[(size_t)q][(size_t)r]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; break; }
		fasim_scan_stats& st = out[(size_t)q][(size_t)r]->stats;
		for (int d = 0; d < nd; d++) {
			const fasim_scan_stats& x = part[(size_t)d][k]->stats;
			st.segments += x.segments; st.segments_skipped += x.segments_skipped; st.units += x.units; st.candidates += x.candidates;
			st.align_calls += x.align_calls; st.logical_cells += x.logical_cells; st.cells_stage2 += x.cells_stage2;
		}
	}
	// tracks and peaks of the device shards: maximum / (value, position, encoding) order
	for (int q = 0; q < nq && !bad && with_track; q++) for (int r = 0; r < nrec && !bad; r++) {
		const size_t k = (size_t)q * nrec + r;
		if (nd == 1) { tracks[(size_t)q][(size_t)r] = tpart[0][k]; tpart[0][k] = nullptr; continue; }
		std::vector<const fasim_track*> tp((size_t)nd);
		for (int d = 0; d < nd; d++) tp[(size_t)d] = tpart[(size_t)d][k];
		if (fasim_track_merge(tp.data(), nd, &tracks[(size_t)q][(size_t)r]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	if (!bad && with_peaks) {
		peaks.resize(nout * 4);
		std::vector<const fasim_peak*> pp((size_t)nd);
		for (int d = 0; d < nd; d++) pp[(size_t)d] = ppart[(size_t)d].data();
		if (fasim_peaks_merge(pp.data(), nd, (int64_t)(nout * 4), peaks.data()) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (int q = 0; q < nq && !bad && profs; q++) {
		if (nd == 1) { (*profs)[(size_t)q] = fpart[0][(size_t)q]; fpart[0][(size_t)q] = nullptr; continue; }
		std::vector<const fasim_tfo_profile*> fp((size_t)nd);
		for (int d = 0; d < nd; d++) fp[(size_t)d] = fpart[(size_t)d][(size_t)q];
		if (fasim_tfo_profile_merge(fp.data(), nd, &(*profs)[(size_t)q]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	// histograms of the device shards: sums, the overlaps at the shard boundaries counted once
	for (size_t k = 0; hists && !bad && k < hists->size(); k++) {
		if (nd == 1) { (*hists)[k] = gpart[0][k]; gpart[0][k] = nullptr; continue; }
		std::vector<const fasim_hist*> hp((size_t)nd);
		for (int d = 0; d < nd; d++) hp[(size_t)d] = gpart[(size_t)d][k];
		if (fasim_hist_merge(hp.data(), nd, &(*hists)[k]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (auto& v : gpart) for (fasim_hist* x : v) fasim_hist_free(x);
	if (bad && hists) for (fasim_hist*& x : *hists) { fasim_hist_free(x); x = nullptr; }
	for (size_t k = 0; counts && !bad && k < counts->size(); k++) {
		if (nd == 1) { (*counts)[k] = cpart[0][k]; cpart[0][k] = nullptr; continue; }
		std::vector<const fasim_site_counts*> cp((size_t)nd);
		for (int d = 0; d < nd; d++) cp[(size_t)d] = cpart[(size_t)d][k];
		if (fasim_site_counts_merge(cp.data(), nd, &(*counts)[k]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (auto& v : cpart) for (fasim_site_counts* x : v) fasim_site_counts_free(x);
	if (bad && counts) for (fasim_site_counts*& x : *counts) { fasim_site_counts_free(x); x = nullptr; }
	// site lists of the device shards: union of the intervals, joined again
	for (int q = 0; q < nq && !bad && sites; q++) for (int r = 0; r < nrec && !bad; r++) {
		const size_t k = (size_t)q * nrec + r;
		if (nd == 1) { (*sites)[(size_t)q][(size_t)r] = spart[0][k]; spart[0][k] = nullptr; continue; }
		std::vector<const fasim_sites*> sp((size_t)nd);
		for (int d = 0; d < nd; d++) sp[(size_t)d] = spart[(size_t)d][k];
		if (fasim_sites_merge(sp.data(), nd, &(*sites)[(size_t)q][(size_t)r]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	// their hits: the part whose site wins supplies the hit
	for (int q = 0; q < nq && !bad && sites && hits; q++) for (int r = 0; r < nrec && !bad; r++) {
		const size_t k = (size_t)q * nrec + r;
		if (nd == 1) { (*hits)[(size_t)q][(size_t)r] = hpart[0][k]; hpart[0][k] = nullptr; continue; }
		std::vector<const fasim_sites*> sp((size_t)nd); std::vector<const fasim_site_hits*> hp((size_t)nd);
		for (int d = 0; d < nd; d++) { sp[(size_t)d] = spart[(size_t)d][k]; hp[(size_t)d] = hpart[(size_t)d][k]; }
		if (fasim_site_hits_merge(sp.data(), hp.data(), nd, nullptr, &(*hits)[(size_t)q][(size_t)r]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
	}
	for (auto& v : hpart) for (fasim_site_hits* x : v) fasim_site_hits_free(x);
	if (bad && hits) for (auto& v : *hits) for (fasim_site_hits*& x : v) { fasim_site_hits_free(x); x = nullptr; }
	for (auto& v : spart) for (fasim_sites* x : v) fasim_sites_free(x);
	if (bad && sites) for (auto& v : *sites) for (fasim_sites*& x : v) { fasim_sites_free(x); x = nullptr; }
	for (auto& v : fpart) for (fasim_tfo_profile* x : v) fasim_tfo_profile_free(x);
	for (auto& v : part) for (fasim_result* x : v) fasim_result_free(x);
	for (auto& v : tpart) for (fasim_track* x : v) fasim_track_free(x);
	if (bad && profs) for (fasim_tfo_profile*& x : *profs) { fasim_tfo_profile_free(x); x = nullptr; }
	if (bad) {
		for (auto& v : out) for (fasim_result*& x : v) { fasim_result_free(x); x = nullptr; }
		for (auto& v : tracks) for (fasim_track*& x : v) { fasim_track_free(x); x = nullptr; }
	}
	return bad;
}

// Host threads for the tails of grouped records (clustering, texts, file writes): FIFO, while the next group is read and scanned.
struct TailPool {
	std::mutex mu; std::condition_variable cv, idle;
	std::deque<std::function<void()>> jobs;
	std::vector<std::thread> th;
	int running = 0; bool stop = false;
	explicit TailPool(int n)
	{
		for (int k = 0; k < n; k++) th.emplace_back([this] {
			for (;;) {
				std::function<void()> job;
				{
					std::unique_lock<std::mutex> lk(mu);
					cv.wait(lk, [&] { return stop || !jobs.empty(); });
					if (jobs.empty()) return;
					job = std::move(jobs.front()); jobs.pop_front(); running++;
				}
				job();
				{ std::lock_guard<std::mutex> lk(mu); running--; if (jobs.empty() && !running) idle.notify_all(); }
			}
		});
	}
	void add(std::function<void()> job) { { std::lock_guard<std::mutex> lk(mu); jobs.push_back(std::move(job)); } cv.notify_one(); }
	void drain() { std::unique_lock<std::mutex> lk(mu); idle.wait(lk, [&] { return jobs.empty() && !running; }); }
	~TailPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto& t : th) t.join(); }
};

// --variants: every (VCF line, ALT allele) scored by the triplex potential through it (fasim_score_variants).
// The genome is streamed record by record; a variant goes to the first record of its chromosome (file order, the header rules of
// --regions) that contains [POS - 1, POS - 1 + len(REF)), and the record's letters there must equal REF.  Per lncRNA one table,
// <O>/<lnc>-<f1 minus 3 chars>.variants.tsv.  Exit status 2: a malformed VCF (nothing written, no device opened); 1: variants that no
// record contains, whose REF differs or whose alleles cannot be scored (NA lines; listed on stderr).
// --variant-hits: the alignment behind every score as well (fasim_score_variants_aligned, section 21), one more table per lncRNA,
// <O>/<lnc>-<f1 minus 3 chars>.variants.hits.tsv; the hits of the records' calls are gathered into one list in the VCF's order.
struct HitGather {
	std::vector<fasim_triplex> t; std::vector<int32_t> qb, qe, tb, te, clen; std::vector<int64_t> coff; std::vector<uint32_t> cigar; std::vector<char> pool;
	int64_t unaligned = 0;
	explicit HitGather(int64_t nvar) : t((size_t)nvar * 8), qb((size_t)nvar * 8, -1), qe((size_t)nvar * 8, -1), tb((size_t)nvar * 8, -1), te((size_t)nvar * 8, -1),
		clen((size_t)nvar * 8, 0), coff((size_t)nvar * 8, 0), pool(1, '\0') { if (!t.empty()) memset(t.data(), 0, t.size() * sizeof(fasim_triplex)); }
	// the eight hits of variant `from` of h become those of variant `to`
	void take(const fasim_site_hits* h, int64_t from, int64_t to)
	{
		for (int s = 0; s < 8; s++) {
			const size_t a = (size_t)from * 8 + (size_t)s, b = (size_t)to * 8 + (size_t)s;
			t[b] = h->t[a]; t[b].seg = (int32_t)to;
			qb[b] = h->q_begin[a]; qe[b] = h->q_end[a]; tb[b] = h->t_begin[a]; te[b] = h->t_end[a]; clen[b] = h->cigar_len[a];
			coff[b] = (int64_t)cigar.size();
			if (h->cigar_len[a] < 0) unaligned++;
			if (h->cigar_len[a] <= 0) { t[b].tfo_off = t[b].tts_off = 0; continue; }
			cigar.insert(cigar.end(), h->cigar + h->cigar_off[a], h->cigar + h->cigar_off[a] + h->cigar_len[a]);
			const char* tfo = h->pool + h->t[a].tfo_off; const char* tts = h->pool + h->t[a].tts_off;
			t[b].tfo_off = (int64_t)pool.size(); pool.insert(pool.end(), tfo, tfo + strlen(tfo) + 1);
			t[b].tts_off = (int64_t)pool.size(); pool.insert(pool.end(), tts, tts + strlen(tts) + 1);
		}
	}
	fasim_site_hits view()
	{
		if (cigar.empty()) cigar.push_back(0);
		fasim_site_hits h;
		h.n = (int64_t)t.size(); h.t = t.data(); h.q_begin = qb.data(); h.q_end = qe.data(); h.t_begin = tb.data(); h.t_end = te.data();
		h.cigar_off = coff.data(); h.cigar_len = clen.data(); h.cigar = cigar.data(); h.pool = pool.data(); h.pool_len = (int64_t)pool.size(); h.unaligned = unaligned;
		return h;
	}
};

static int run_variants(const std::string& vcf_path, int flank, const std::string& f1, const std::string& f2, const std::string& outdir, int device,
	bool upper, const fasim_params& p, bool want_hits, const std::string& sample)
{
	fasim_variant* vars = nullptr; int64_t nvar = 0;
	fasim_genotype* gts = nullptr;
	const bool want_haps = !sample.empty();
	if ((want_haps ? fasim_read_vcf_sample(vcf_path.c_str(), sample.c_str(), &vars, &nvar, &gts) : fasim_read_vcf(vcf_path.c_str(), &vars, &nvar)) != FASIM_OK) {
		fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 2;
	}
	std::unique_ptr<fasim_variant, void (*)(void*)> owner(vars, fasim_free);
	std::unique_ptr<fasim_genotype, void (*)(void*)> gowner(gts, fasim_free);
	std::vector<Rna> rnas;
	DnaReader reader;
	reader.upper = upper;
	if (!reader.open(f1)) { fprintf(stderr, "fasim: cannot read DNA file %s\n", f1.c_str()); return 1; }
	if (!read_rnas(f2, rnas)) { fprintf(stderr, "fasim: cannot read RNA file %s\n", f2.c_str()); return 1; }
	for (const Rna& r : rnas) if (r.seq.empty() || r.seq.size() > (size_t)FASIM_MAX_QUERY) {
		fprintf(stderr, "fasim: RNA record '%s' in %s has %zu nt: a query has 1 to %d nt\n", r.name.c_str(), f2.c_str(), r.seq.size(), FASIM_MAX_QUERY);
		return 1;
	}
	std::cout << "Searching triplexes using Fasim" << std::endl;
	for (const Rna& r : rnas) std::cout << r.name << std::endl;
	const int nq = (int)rnas.size();
	std::vector<const char*> qp((size_t)nq); std::vector<int32_t> ql((size_t)nq);
	for (int q = 0; q < nq; q++) { qp[(size_t)q] = rnas[(size_t)q].seq.data(); ql[(size_t)q] = (int32_t)rnas[(size_t)q].seq.size(); }
	// state of an entry: 0 not met, 1 scored, 2 REF differs, 3 unusable alleles
	std::vector<uint8_t> state((size_t)nvar, 0);
	std::vector<std::vector<fasim_variant_score>> scores((size_t)nq, std::vector<fasim_variant_score>((size_t)nvar));
	std::vector<std::vector<fasim_hap_score>> haps(want_haps ? (size_t)nq : 0, std::vector<fasim_hap_score>((size_t)nvar));
	std::vector<fasim_variant_window> windows(want_hits ? (size_t)nvar : 0);
	std::vector<HitGather> gathered;
	if (want_hits) { memset(windows.data(), 0, windows.size() * sizeof(fasim_variant_window)); for (int q = 0; q < nq; q++) gathered.emplace_back(nvar); }
	std::map<std::string, std::multimap<int64_t, int64_t>> todo;
	std::set<std::string> chroms_seen;
	for (int64_t k = 0; k < nvar; k++) {
		if (vars[k].alt_len < 0) state[(size_t)k] = 3;
		// (an entry that cannot be scored still says what a haplotype carries on its line: --sample hands it on, unscored)
		if (vars[k].alt_len >= 0 || want_haps) todo[vars[k].chrom].emplace(vars[k].pos, k);
	}
	fasim_engine* eng = nullptr;
	DnaRecord rec;
	size_t nrec = 0;
	while (reader.next(rec)) {
		std::string chrom = rec.chr; int64_t rs = (int64_t)rec.start - 1;
		const size_t w0 = rec.header.find_first_not_of("> \t\r");
		const std::string word = w0 == std::string::npos ? std::string() : rec.header.substr(w0, rec.header.find_first_of(" \t\r", w0) - w0);
		if (word.find('|') == std::string::npos) { chrom = word; rs = 0; }
		nrec++;
		chroms_seen.insert(chrom);
		auto it = todo.find(chrom);
		if (it == todo.end()) continue;
		const int64_t re = rs + (int64_t)rec.seq.size();
		std::vector<int64_t> mine;
		for (auto j = it->second.lower_bound(rs); j != it->second.end() && j->first < re; ) {
			const fasim_variant& x = vars[j->second];
			if (x.pos + x.ref_len > re) { ++j; continue; }
			if (x.alt_len >= 0 && memcmp(rec.seq.data() + (x.pos - rs), x.ref, (size_t)x.ref_len) != 0) state[(size_t)j->second] = 2;
			else mine.push_back(j->second);
			j = it->second.erase(j);
		}
		if (mine.empty()) continue;
		std::sort(mine.begin(), mine.end());
		std::vector<fasim_variant> loc(mine.size());
		for (size_t k = 0; k < mine.size(); k++) { loc[k] = vars[mine[k]]; loc[k].pos -= rs; loc[k].rec = 0; }
		if (!eng && fasim_engine_create(device, &eng) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		const int64_t off0 = 0, len0 = (int64_t)rec.seq.size();
		std::vector<fasim_variant_score> got((size_t)nq * mine.size());
		std::vector<fasim_variant_window> wloc(want_hits ? mine.size() : 0);
		std::vector<fasim_site_hits*> hloc(want_hits ? (size_t)nq : 0, nullptr);
		const int rc = want_hits
			? fasim_score_variants_aligned(eng, qp.data(), ql.data(), nq, rec.seq.data(), &off0, &len0, 1, loc.data(), (int64_t)loc.size(), flank, &p, got.data(), nullptr, wloc.data(), hloc.data())
			: fasim_score_variants(eng, qp.data(), ql.data(), nq, rec.seq.data(), &off0, &len0, 1, loc.data(), (int64_t)loc.size(), flank, &p, got.data(), nullptr);
		if (rc != FASIM_OK) {
			fprintf(stderr, "fasim: %s\n", fasim_last_error(eng));
			fasim_engine_destroy(eng);
			return 1;
		}
		if (want_hits) {
			for (size_t k = 0; k < mine.size(); k++) windows[(size_t)mine[k]] = wloc[k];
			for (int q = 0; q < nq; q++) {
				for (size_t k = 0; k < mine.size(); k++) gathered[(size_t)q].take(hloc[(size_t)q], (int64_t)k, mine[k]);
				fasim_site_hits_free(hloc[(size_t)q]);
			}
		}
		for (int q = 0; q < nq; q++) for (size_t k = 0; k < mine.size(); k++) scores[(size_t)q][(size_t)mine[k]] = got[(size_t)q * mine.size() + k];
		if (want_haps) {
			// the record's matched entries with their genotypes: nothing else is ever applied as a neighbour
			std::vector<fasim_genotype> gloc(mine.size());
			for (size_t k = 0; k < mine.size(); k++) gloc[k] = gts[mine[k]];
			std::vector<fasim_hap_score> hgot((size_t)nq * mine.size());
			if (fasim_score_haplotypes(eng, qp.data(), ql.data(), nq, rec.seq.data(), &off0, &len0, 1, loc.data(), gloc.data(), nullptr, (int64_t)loc.size(), flank, &p, hgot.data(), nullptr) != FASIM_OK) {
				fprintf(stderr, "fasim: %s\n", fasim_last_error(eng));
				fasim_engine_destroy(eng);
				return 1;
			}
			for (int q = 0; q < nq; q++) for (size_t k = 0; k < mine.size(); k++) haps[(size_t)q][(size_t)mine[k]] = hgot[(size_t)q * mine.size() + k];
		}
		for (int64_t k : mine) if (state[(size_t)k] != 3) state[(size_t)k] = 1;
	}
	if (eng) fasim_engine_destroy(eng);
	if (nrec == 0) { fprintf(stderr, "fasim: no record in DNA file %s\n", f1.c_str()); return 1; }
	const std::string base = f1.substr(0, f1.size() >= 3 ? f1.size() - 3 : 0);
	std::vector<uint8_t> matched((size_t)nvar);
	for (int64_t k = 0; k < nvar; k++) matched[(size_t)k] = state[(size_t)k] == 1;
	int bad = 0;
	for (int q = 0; q < nq; q++) {
		char* text = nullptr; int64_t len = 0;
		if (fasim_variants_tsv(vars, scores[(size_t)q].data(), nvar, flank, rnas[(size_t)q].name.c_str(), matched.data(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		bad |= write_file(outdir + "/" + rnas[(size_t)q].name + "-" + base + ".variants.tsv", text, len);
		fasim_free(text);
		if (want_haps) {
			text = nullptr; len = 0;
			if (fasim_haplotypes_tsv(vars, gts, haps[(size_t)q].data(), nvar, flank, rnas[(size_t)q].name.c_str(), sample.c_str(), matched.data(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			bad |= write_file(outdir + "/" + rnas[(size_t)q].name + "-" + base + ".haplotypes.tsv", text, len);
			fasim_free(text);
		}
		if (!want_hits) continue;
		const fasim_site_hits view = gathered[(size_t)q].view();
		text = nullptr; len = 0;
		if (fasim_variant_hits_tsv(vars, scores[(size_t)q].data(), windows.data(), &view, nvar, flank, rnas[(size_t)q].name.c_str(), matched.data(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		bad |= write_file(outdir + "/" + rnas[(size_t)q].name + "-" + base + ".variants.hits.tsv", text, len);
		fasim_free(text);
	}
	if (bad) return 1;
	size_t lost = 0;
	for (int64_t k = 0; k < nvar; k++) {
		if (state[(size_t)k] == 1) continue;
		const fasim_variant& x = vars[k];
		const char* why = state[(size_t)k] == 3 ? "its alleles cannot be scored (1 to 1024 letters of ACGTN each)" : state[(size_t)k] == 2 ? "REF differs from the DNA record"
			: chroms_seen.count(x.chrom) ? "no DNA record of its chromosome contains it" : "no DNA record of its chromosome";
		if (lost++ < 20) fprintf(stderr, "fasim: VCF line %lld %s:%lld: %s\n", (long long)x.line, x.chrom, (long long)(x.pos + 1), why);
	}
	if (lost > 20) fprintf(stderr, "fasim: ... and %zu more\n", lost - 20);
	if (lost) { fprintf(stderr, "fasim: %zu of %lld variants were not scored (NA in the table)\n", lost, (long long)nvar); return 1; }
	std::cout << "finished normally" << std::endl;
	return 0;
}

// --mutagenesis: every substitution at every position of the BED intervals (fasim_score_mutagenesis).  The BED
// file is read and checked before anything else; the genome is streamed record by record and an interval goes to the first record of
// its chromosome that holds it entirely (the rules of --regions).  Per lncRNA one table, <O>/<lnc>-<f1 minus 3 chars>.mutagenesis.tsv.
// Exit status 2: a bad BED file or an interval too long for the flank (nothing written, no device opened); 1: intervals that no
// record contains (listed as --regions lists them; the others are written).
static int run_mutagenesis(const std::string& bed_path, int flank, const std::string& f1, const std::string& f2, const std::string& outdir, int device,
	bool upper, const fasim_params& p, const std::vector<int32_t>& del_lengths, bool del_only)
{
	const int nlen = (int)del_lengths.size();
	fasim_region* reg = nullptr; int64_t nreg = 0;
	if (fasim_read_bed(bed_path.c_str(), &reg, &nreg) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 2; }
	std::unique_ptr<fasim_region, void (*)(void*)> owner(reg, fasim_free);
	for (int64_t k = 0; k < nreg; k++) if (reg[k].end - reg[k].start + 2 * (int64_t)flank > 5120) {
		fprintf(stderr, "fasim: BED line %lld (%s): %lld positions and two flanks of %d are more than 5120 columns: --mutagenesis takes intervals of at most %d nt with this flank\n",
			(long long)reg[k].line, reg[k].name, (long long)(reg[k].end - reg[k].start), flank, 5120 - 2 * flank);
		return 2;
	}
	std::vector<Rna> rnas;
	DnaReader reader;
	reader.upper = upper;
	if (!reader.open(f1)) { fprintf(stderr, "fasim: cannot read DNA file %s\n", f1.c_str()); return 1; }
	if (!read_rnas(f2, rnas)) { fprintf(stderr, "fasim: cannot read RNA file %s\n", f2.c_str()); return 1; }
	for (const Rna& r : rnas) if (r.seq.empty() || r.seq.size() > (size_t)FASIM_MAX_QUERY) {
		fprintf(stderr, "fasim: RNA record '%s' in %s has %zu nt: a query has 1 to %d nt\n", r.name.c_str(), f2.c_str(), r.seq.size(), FASIM_MAX_QUERY);
		return 1;
	}
	std::cout << "Searching triplexes using Fasim" << std::endl;
	for (const Rna& r : rnas) std::cout << r.name << std::endl;
	const int nq = (int)rnas.size();
	std::vector<const char*> qp((size_t)nq); std::vector<int32_t> ql((size_t)nq);
	for (int q = 0; q < nq; q++) { qp[(size_t)q] = rnas[(size_t)q].seq.data(); ql[(size_t)q] = (int32_t)rnas[(size_t)q].seq.size(); }
	// per lncRNA and interval the scores of its positions; empty: not met
	std::vector<std::vector<std::vector<fasim_mut_score>>> scores((size_t)nq, std::vector<std::vector<fasim_mut_score>>((size_t)nreg));
	// --deletions: per lncRNA and interval the scores of its (position, length) pairs, and per interval its letters
	std::vector<std::vector<std::vector<fasim_del_score>>> dscores((size_t)nq, std::vector<std::vector<fasim_del_score>>((size_t)nreg));
	std::vector<std::string> seqs((size_t)nreg);
	std::vector<char> met((size_t)nreg, 0);
	std::map<std::string, std::multimap<int64_t, int64_t>> todo;
	std::set<std::string> chroms_seen;
	std::vector<char> held_start((size_t)nreg, 0);
	for (int64_t k = 0; k < nreg; k++) todo[reg[k].chrom].emplace(reg[k].start, k);
	fasim_engine* eng = nullptr;
	DnaRecord rec;
	size_t nrec = 0;
	while (reader.next(rec)) {
		std::string chrom = rec.chr; int64_t rs = (int64_t)rec.start - 1;
		const size_t w0 = rec.header.find_first_not_of("> \t\r");
		const std::string word = w0 == std::string::npos ? std::string() : rec.header.substr(w0, rec.header.find_first_of(" \t\r", w0) - w0);
		if (word.find('|') == std::string::npos) { chrom = word; rs = 0; }
		nrec++;
		chroms_seen.insert(chrom);
		auto it = todo.find(chrom);
		if (it == todo.end()) continue;
		const int64_t re = rs + (int64_t)rec.seq.size();
		std::vector<int64_t> mine;
		for (auto j = it->second.lower_bound(rs); j != it->second.end() && j->first < re; ) {
			if (reg[j->second].end <= re) { mine.push_back(j->second); j = it->second.erase(j); }
			else { held_start[(size_t)j->second] = 1; ++j; }
		}
		if (mine.empty()) continue;
		std::sort(mine.begin(), mine.end());
		std::vector<fasim_interval> loc(mine.size());
		int64_t npos = 0;
		for (size_t k = 0; k < mine.size(); k++) {
			const fasim_region& g = reg[mine[k]];
			loc[k].rec = 0; loc[k].reserved = 0; loc[k].start = g.start - rs; loc[k].end = g.end - rs;
			npos += g.end - g.start;
		}
		if (!eng && fasim_engine_create(device, &eng) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		const int64_t off0 = 0, len0 = (int64_t)rec.seq.size();
		std::vector<fasim_mut_score> got(del_only ? 0 : (size_t)nq * (size_t)npos);
		if (!del_only && fasim_score_mutagenesis(eng, qp.data(), ql.data(), nq, rec.seq.data(), &off0, &len0, 1, loc.data(), (int64_t)loc.size(), flank, &p, got.data(), nullptr) != FASIM_OK) {
			fprintf(stderr, "fasim: %s\n", fasim_last_error(eng));
			fasim_engine_destroy(eng);
			return 1;
		}
		std::vector<fasim_del_score> dgot((size_t)nq * (size_t)npos * (size_t)nlen);
		if (nlen && fasim_score_deletions(eng, qp.data(), ql.data(), nq, rec.seq.data(), &off0, &len0, 1, loc.data(), (int64_t)loc.size(), flank, del_lengths.data(), nlen, &p, dgot.data(), nullptr) != FASIM_OK) {
			fprintf(stderr, "fasim: %s\n", fasim_last_error(eng));
			fasim_engine_destroy(eng);
			return 1;
		}
		for (size_t k = 0; k < mine.size(); k++) {
			met[(size_t)mine[k]] = 1;
			if (nlen) seqs[(size_t)mine[k]].assign(rec.seq.data() + loc[k].start, (size_t)(loc[k].end - loc[k].start));
		}
		for (int q = 0; q < nq; q++) {
			size_t at = (size_t)q * (size_t)npos;
			for (size_t k = 0; k < mine.size(); k++) {
				const size_t len = (size_t)(reg[mine[k]].end - reg[mine[k]].start);
				if (!del_only) scores[(size_t)q][(size_t)mine[k]].assign(got.begin() + (ptrdiff_t)at, got.begin() + (ptrdiff_t)(at + len));
				if (nlen) dscores[(size_t)q][(size_t)mine[k]].assign(dgot.begin() + (ptrdiff_t)(at * (size_t)nlen), dgot.begin() + (ptrdiff_t)((at + len) * (size_t)nlen));
				at += len;
			}
		}
	}
	if (eng) fasim_engine_destroy(eng);
	if (nrec == 0) { fprintf(stderr, "fasim: no record in DNA file %s\n", f1.c_str()); return 1; }
	const std::string base = f1.substr(0, f1.size() >= 3 ? f1.size() - 3 : 0);
	int bad = 0;
	for (int q = 0; q < nq && nlen; q++) {
		std::vector<int64_t> offsets((size_t)nreg + 1, 0);
		std::vector<fasim_del_score> all;
		std::vector<const char*> letters((size_t)nreg, nullptr);
		for (int64_t k = 0; k < nreg; k++) {
			all.insert(all.end(), dscores[(size_t)q][(size_t)k].begin(), dscores[(size_t)q][(size_t)k].end());
			offsets[(size_t)k + 1] = offsets[(size_t)k] + (met[(size_t)k] ? reg[k].end - reg[k].start : 0);
			letters[(size_t)k] = seqs[(size_t)k].c_str();
		}
		char* text = nullptr; int64_t len = 0;
		if (fasim_deletions_tsv(reg, offsets.data(), nreg, all.data(), letters.data(), del_lengths.data(), nlen, flank, rnas[(size_t)q].name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		bad |= write_file(outdir + "/" + rnas[(size_t)q].name + "-" + base + ".deletions.tsv", text, len);
		fasim_free(text);
	}
	for (int q = 0; q < nq && !del_only; q++) {
		std::vector<int64_t> offsets((size_t)nreg + 1, 0);
		std::vector<fasim_mut_score> all;
		for (int64_t k = 0; k < nreg; k++) {
			all.insert(all.end(), scores[(size_t)q][(size_t)k].begin(), scores[(size_t)q][(size_t)k].end());
			offsets[(size_t)k + 1] = (int64_t)all.size();
		}
		char* text = nullptr; int64_t len = 0;
		if (fasim_mutagenesis_tsv(reg, offsets.data(), nreg, all.data(), flank, rnas[(size_t)q].name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		bad |= write_file(outdir + "/" + rnas[(size_t)q].name + "-" + base + ".mutagenesis.tsv", text, len);
		fasim_free(text);
	}
	if (bad) return 1;
	std::vector<std::pair<int64_t, std::string>> lost;
	for (const auto& c : todo) for (const auto& j : c.second) {
		const fasim_region& g = reg[j.second];
		const char* why = held_start[(size_t)j.second] ? "runs past the end of the DNA record that holds its start"
			: chroms_seen.count(g.chrom) ? "no DNA record of its chromosome holds it" : "no DNA record of its chromosome";
		char buf[512];
		snprintf(buf, sizeof buf, "fasim: BED line %lld (%s) %s:%lld-%lld: %s\n", (long long)g.line, g.name, g.chrom, (long long)g.start, (long long)g.end, why);
		lost.emplace_back(j.second, buf);
	}
	if (!lost.empty()) {
		std::sort(lost.begin(), lost.end());      // in BED order
		for (size_t k = 0; k < lost.size() && k < 20; k++) fputs(lost[k].second.c_str(), stderr);
		if (lost.size() > 20) fprintf(stderr, "fasim: ... and %zu more\n", lost.size() - 20);
		fprintf(stderr, "fasim: %zu of %lld BED intervals lie in no DNA record of %s: they have no lines in the table\n", lost.size(), (long long)nreg, f1.c_str());
		return 1;
	}
	std::cout << "finished normally" << std::endl;
	return 0;
}

int main(int argc, char* const* argv)
{
	fasim_params p; fasim_params_default(&p);
	std::string f1 = "./", f2 = "./", outdir = "./", bed_path, vcf_path, sample;
	bool sample_given = false;
	bool devices_given = false, flank_given = false, variant_hits = false; int variant_flank = 300;
	std::string mut_path; bool mut_flank_given = false; int mut_flank = 300;
	std::string del_list; bool del_given = false, del_only = false;
	std::vector<int> devices(1, 0);
	bool stats = false, all_records = false, accumulate = false, upper = false, track = false, screen = false, screen_only = false;
	bool sites = false, sites_gap_given = false, hist_arg_given = false, hist_arg_bad = false, hist_shuffle_bad = false;
	TrackOpt trk;
	int tail_flags = 0;
	const char* optstring = "f:s:r:O:c:m:t:i:S:z:Y:Z:h:C:D:E:o:y:Fd";
	struct option lo[] = {
		{ "f1", required_argument, NULL, 'f' }, { "f2", required_argument, NULL, 's' }, { "ni", required_argument, NULL, 'y' },
		{ "na", required_argument, NULL, 'z' }, { "pc", required_argument, NULL, 'Y' }, { "pt", required_argument, NULL, 'Z' },
		{ "cn", required_argument, NULL, 'C' }, { "ds", required_argument, NULL, 'D' }, { "lg", required_argument, NULL, 'E' },
		{ "device", required_argument, NULL, 1001 }, { "stats", no_argument, NULL, 1002 }, { "all-records", no_argument, NULL, 1003 },
		{ "devices", required_argument, NULL, 1004 }, { "accumulate-records", no_argument, NULL, 1005 }, { "upper", no_argument, NULL, 1006 },
		{ "clamp-cluster", no_argument, NULL, 1007 }, { "regions", required_argument, NULL, 1008 },
		{ "track", required_argument, NULL, 1009 }, { "track-min", required_argument, NULL, 1010 }, { "track-only", no_argument, NULL, 1011 },
		{ "screen", no_argument, NULL, 1012 }, { "screen-only", no_argument, NULL, 1013 },
		{ "tfo-profile", no_argument, NULL, 1014 }, { "tfo-profile-only", no_argument, NULL, 1015 },
		{ "sites", required_argument, NULL, 1016 }, { "sites-gap", required_argument, NULL, 1017 }, { "sites-only", no_argument, NULL, 1018 }, { "sites-align", no_argument, NULL, 1019 }, { "oligos", no_argument, NULL, 1020 }, { "oligo-hits", no_argument, NULL, 1026 }, { "oligo-profile", no_argument, NULL, 1032 }, { "oligo-screen", no_argument, NULL, 1033 },
		{ "potential-hist", no_argument, NULL, 1021 }, { "hist-controls", required_argument, NULL, 1022 }, { "hist-seed", required_argument, NULL, 1023 },
		{ "hist-fdr", required_argument, NULL, 1024 }, { "potential-hist-only", no_argument, NULL, 1025 },
		{ "hist-sites", no_argument, NULL, 1030 }, { "hist-shuffle", required_argument, NULL, 1031 },
		{ "variants", required_argument, NULL, 1027 }, { "variant-flank", required_argument, NULL, 1028 },
		{ "variant-hits", no_argument, NULL, 1029 }, { "sample", required_argument, NULL, 1034 },
		{ "mutagenesis", required_argument, NULL, 1035 }, { "mutagenesis-flank", required_argument, NULL, 1036 },
		{ "deletions", required_argument, NULL, 1037 }, { "deletions-only", no_argument, NULL, 1038 }, { 0, 0, 0, 0 } };
	int opt;
	while ((opt = getopt_long_only(argc, argv, optstring, lo, NULL)) != -1) {
		switch (opt) {
		case 'f': f1 = optarg; break;
		case 's': f2 = optarg; break;
		case 'r': p.rule = atoi(optarg); break;
		case 'O': outdir = optarg; break;
		case 'c': p.cutLength = atoi(optarg); break;
		case 'm': break;                                  // minScore: parsed and unused by the reference
		case 't': p.strand = atoi(optarg); break;
		case 'i': p.minIdentity = atoi(optarg); break;    // sic: atoi (B10)
		case 'S': p.minStability = atoi(optarg); break;   // sic: atoi (B10)
		case 'y': p.ntMin = atoi(optarg); break;
		case 'z': p.ntMax = atoi(optarg); break;
		case 'Y': p.penaltyC = atoi(optarg); break;
		case 'Z': p.penaltyT = atoi(optarg); break;
		case 'o': p.overlapLength = atoi(optarg); break;
		case 'D': p.cDistance = atoi(optarg); break;
		case 'E': p.cLength = atoi(optarg); break;
		case 'C': break;                                  // -cn only picked a result vector in the reference (:129-163); see --devices
		case 'F': p.classicSim = 1; break;                // doFastSim = false (Fasim-LongTarget.cpp:360-362): SIM() instead of fastSIM()
		case 'd': break;
		case 1001: devices.assign(1, atoi(optarg)); break;
		case 1002: stats = true; break;
		case 1003: all_records = true; break;
		case 1027: vcf_path = optarg; break;
		case 1028: flank_given = true; variant_flank = strict_int(optarg, -1); break;
		case 1029: variant_hits = true; break;
		case 1034: sample_given = true; sample = optarg; break;
		case 1035: mut_path = optarg; break;
		case 1036: mut_flank_given = true; mut_flank = strict_int(optarg, -1); break;
		case 1037: del_given = true; del_list = optarg; break;
		case 1038: del_only = true; break;
		case 1004: devices_given = true; devices = parse_devices(optarg); if (devices.empty()) { fprintf(stderr, "fasim: bad --devices list\n"); return 2; } break;
		case 1005: accumulate = true; break;
		case 1006: upper = true; break;
		case 1007: tail_flags |= FASIM_TAIL_CLAMP_CLUSTER; break;
		case 1008: bed_path = optarg; break;
		case 1009: track = true; trk.bin = atoi(optarg); break;
		case 1010: trk.min_value = atoi(optarg); break;
		case 1011: trk.only = true; break;
		case 1012: screen = true; break;
		case 1013: screen = screen_only = true; break;
		case 1014: trk.tfo = true; break;
		case 1015: trk.tfo = trk.tfo_only = true; break;
		case 1016: sites = true; trk.sites = strict_int(optarg, 0); break;           // (0 and -1: refused below as out of range)
		case 1017: sites_gap_given = true; trk.sites_gap = strict_int(optarg, -1); break;
		case 1018: trk.sites_only = true; break;
		case 1019: trk.sites_align = true; break;
		case 1020: trk.oligos = true; break;
		case 1026: trk.oligo_hits = true; break;
		case 1032: trk.oligo_profile = true; break;
		case 1033: trk.oligo_screen = true; break;
		case 1021: trk.hist = true; break;
		case 1022: hist_arg_given = true; trk.hist_controls = strict_int(optarg, -1); break;
		case 1023: { hist_arg_given = true; char* end = nullptr; errno = 0; trk.hist_seed = strtoull(optarg, &end, 10); if (end == optarg || *end != '\0' || errno == ERANGE || optarg[0] == '-') hist_arg_bad = true; break; }
		case 1024: { hist_arg_given = true; char* end = nullptr; trk.hist_fdr = strtod(optarg, &end); if (end == optarg || *end != '\0') trk.hist_fdr = -1.0; break; }
		case 1025: trk.hist_only = true; break;
		case 1030: hist_arg_given = true; trk.hist_sites = true; break;
		case 1031: hist_arg_given = true; if (!strcmp(optarg, "di")) trk.hist_dinuc = true; else if (strcmp(optarg, "mono")) hist_shuffle_bad = true; break;
		default: fprintf(stderr, "usage: fasim -f1 DNA.fa -f2 RNA.fa [-O outdir] [-r R] [-t T] [-lg L] ... [--devices 0-7] [--all-records | --regions FILE.bed] [--upper] [--track BIN [--track-min V] [--track-only]] [--screen | --screen-only] [--tfo-profile | --tfo-profile-only] [--sites V [--sites-gap G] [--sites-only] [--sites-align] [--oligos [--oligo-hits]]] [--oligos [--oligo-profile] [--oligo-screen]] [--potential-hist [--hist-controls K] [--hist-seed S] [--hist-fdr Q] [--potential-hist-only] [--hist-sites] [--hist-shuffle mono|di]] [--variants FILE.vcf [--variant-flank F] [--variant-hits] [--sample NAME]] [--mutagenesis FILE.bed [--mutagenesis-flank F] [--deletions D,D,... [--deletions-only]]]\n"); return 2;
		}
	}
	if (all_records && accumulate) { fprintf(stderr, "fasim: --all-records and --accumulate-records exclude each other\n"); return 2; }
	const bool regions = !bed_path.empty();
	if (regions && (all_records || accumulate)) { fprintf(stderr, "fasim: --regions excludes --all-records and --accumulate-records\n"); return 2; }
	if (trk.only && !track) { fprintf(stderr, "fasim: --track-only needs --track BIN\n"); return 2; }
	if (track && trk.bin < 1) { fprintf(stderr, "fasim: --track needs a bin width of at least 1\n"); return 2; }
	if (track && trk.min_value < 1) { fprintf(stderr, "fasim: --track-min needs a value of at least 1 (bins of value 0 are never written)\n"); return 2; }
	if (track && (regions || accumulate || p.classicSim)) { fprintf(stderr, "fasim: --track is not available with --regions, --accumulate-records or -F\n"); return 2; }
	if (screen && !(regions || all_records)) { fprintf(stderr, "fasim: --screen needs --regions FILE.bed or --all-records\n"); return 2; }
	if (screen && (accumulate || p.classicSim)) { fprintf(stderr, "fasim: --screen is not available with --accumulate-records or -F\n"); return 2; }
	if (screen_only && track) { fprintf(stderr, "fasim: --screen-only writes the screen table only: not with --track\n"); return 2; }
	if (trk.tfo && (p.classicSim || accumulate || track || screen)) { fprintf(stderr, "fasim: --tfo-profile is not available with -F, --accumulate-records, --track or --screen\n"); return 2; }
	if ((sites_gap_given || trk.sites_only || trk.sites_align) && !sites) { fprintf(stderr, "fasim: --sites-gap, --sites-only and --sites-align need --sites V\n"); return 2; }
	if (sites && (trk.sites < 1 || trk.sites > 16383)) { fprintf(stderr, "fasim: --sites needs an integer in [1, 16383]\n"); return 2; }
	if (sites && trk.sites_gap < 0) { fprintf(stderr, "fasim: --sites-gap needs an integer of at least 0\n"); return 2; }
	if (sites && (p.classicSim || accumulate || track || screen || trk.tfo)) { fprintf(stderr, "fasim: --sites is not available with -F, --accumulate-records, --track, --screen or --tfo-profile\n"); return 2; }
	if ((hist_arg_given || trk.hist_only) && !trk.hist) { fprintf(stderr, "fasim: --hist-controls, --hist-seed, --hist-fdr, --hist-sites, --hist-shuffle and --potential-hist-only need --potential-hist\n"); return 2; }
	if (hist_shuffle_bad) { fprintf(stderr, "fasim: --hist-shuffle needs mono or di\n"); return 2; }
	if (trk.hist && (p.classicSim || accumulate || track || screen || trk.tfo || sites)) { fprintf(stderr, "fasim: --potential-hist is not available with -F, --accumulate-records, --track, --screen, --tfo-profile or --sites\n"); return 2; }
	if (trk.hist && trk.hist_controls < 0) { fprintf(stderr, "fasim: --hist-controls needs an integer of at least 0\n"); return 2; }
	if (trk.hist && hist_arg_bad) { fprintf(stderr, "fasim: --hist-seed needs an unsigned integer\n"); return 2; }
	if (trk.hist && !(trk.hist_fdr > 0.0 && trk.hist_fdr <= 1.0)) { fprintf(stderr, "fasim: --hist-fdr needs a number in (0, 1]\n"); return 2; }
	if (trk.hist && 2 * (long long)p.overlapLength > (long long)p.cutLength) { fprintf(stderr, "fasim: --potential-hist needs -o of at most half of -c (a base would lie in three segments)\n"); return 2; }
	const bool panel_extra = trk.oligo_profile || trk.oligo_screen;
	if (panel_extra && !trk.oligos) { fprintf(stderr, "fasim: --oligo-profile and --oligo-screen need --oligos\n"); return 2; }
	if (trk.oligo_screen && !(regions || all_records)) { fprintf(stderr, "fasim: --oligo-screen needs --regions FILE.bed or --all-records\n"); return 2; }
	if (panel_extra && (trk.hist || trk.oligo_hits)) { fprintf(stderr, "fasim: --oligo-profile and --oligo-screen are not available with --potential-hist or --oligo-hits\n"); return 2; }
	if (trk.oligos && !sites && !trk.hist && !panel_extra) { fprintf(stderr, "fasim: --oligos needs --sites V, --potential-hist, --oligo-profile or --oligo-screen\n"); return 2; }
	if (trk.oligos && (trk.sites_align || trk.tfo || p.classicSim || track || screen || accumulate)) { fprintf(stderr, "fasim: --oligos is not available with --sites-align, -F, --track, --screen, --tfo-profile or --accumulate-records\n"); return 2; }
	if (trk.oligo_hits && (!trk.oligos || !sites || trk.hist)) { fprintf(stderr, "fasim: --oligo-hits needs --oligos --sites V (and is not available with --potential-hist)\n"); return 2; }
	const bool variants = !vcf_path.empty();
	if (flank_given && !variants) { fprintf(stderr, "fasim: --variant-flank needs --variants FILE.vcf\n"); return 2; }
	if (variant_hits && !variants) { fprintf(stderr, "fasim: --variant-hits needs --variants FILE.vcf\n"); return 2; }
	if (sample_given && !variants) { fprintf(stderr, "fasim: --sample needs --variants FILE.vcf\n"); return 2; }
	if (sample_given && sample.empty()) { fprintf(stderr, "fasim: --sample needs the name of a sample of the VCF\n"); return 2; }
	if (variants && (variant_flank < 0 || variant_flank > FASIM_MAX_FLANK)) { fprintf(stderr, "fasim: --variant-flank needs an integer in [0, %d]\n", FASIM_MAX_FLANK); return 2; }
	if (variants && (regions || all_records || accumulate || p.classicSim || track || screen || trk.tfo || sites || trk.oligos || trk.hist || devices_given)) {
		fprintf(stderr, "fasim: --variants is not available with --regions, --all-records, --accumulate-records, -F, --track, --screen, --tfo-profile, --sites, --oligos, --potential-hist or --devices\n");
		return 2;
	}
	const bool mutagenesis = !mut_path.empty();
	if (mut_flank_given && !mutagenesis) { fprintf(stderr, "fasim: --mutagenesis-flank needs --mutagenesis FILE.bed\n"); return 2; }
	if (mutagenesis && (mut_flank < 0 || mut_flank > FASIM_MAX_FLANK)) { fprintf(stderr, "fasim: --mutagenesis-flank needs an integer in [0, %d]\n", FASIM_MAX_FLANK); return 2; }
	if (mutagenesis && (variants || regions || all_records || accumulate || p.classicSim || track || screen || trk.tfo || sites || trk.oligos || trk.hist || devices_given)) {
		fprintf(stderr, "fasim: --mutagenesis is not available with --variants, --regions, --all-records, --accumulate-records, -F, --track, --screen, --tfo-profile, --sites, --oligos, --potential-hist or --devices\n");
		return 2;
	}
	if ((del_given || del_only) && !mutagenesis) { fprintf(stderr, "fasim: --deletions and --deletions-only need --mutagenesis FILE.bed\n"); return 2; }
	if (del_only && !del_given) { fprintf(stderr, "fasim: --deletions-only needs --deletions LIST\n"); return 2; }
	std::vector<int32_t> del_lengths;
	if (del_given) {
		size_t at = 0;
		bool ok = !del_list.empty();
		while (ok && at <= del_list.size()) {
			const size_t comma = std::min(del_list.find(',', at), del_list.size());
			const int d = strict_int(del_list.substr(at, comma - at).c_str(), -1);
			ok = d >= 1 && d <= FASIM_MAX_ALLELE - 1 && (del_lengths.empty() || d > del_lengths.back()) && del_lengths.size() < (size_t)FASIM_MAX_DELETION_LENGTHS;
			del_lengths.push_back(d);
			at = comma + 1;
		}
		if (!ok) {
			fprintf(stderr, "fasim: --deletions needs 1 to %d strictly ascending integers in [1, %d], comma-separated\n", FASIM_MAX_DELETION_LENGTHS, FASIM_MAX_ALLELE - 1);
			return 2;
		}
	}
	if (mutagenesis) return run_mutagenesis(mut_path, mut_flank, f1, f2, outdir, devices[0], upper, p, del_lengths, del_only);
	if (variants) return run_variants(vcf_path, variant_flank, f1, f2, outdir, devices[0], upper, p, variant_hits, sample);
	if (trk.oligos) trk.sites_only = true;      // a panel has no triplex records: the sites files and the panel table are all it writes
	if (trk.oligos && trk.hist) trk.hist_only = true;      // (or the oligos' histograms)
	if (!sites) trk.sites = 0;
	trk.peaks = screen || trk.oligo_screen; trk.no_stage3 = screen_only || trk.only || trk.tfo_only || trk.sites_only || trk.hist_only;
	// --regions: the BED file is read and checked before anything else happens (a bad file writes nothing)
	fasim_region* reg = nullptr; int64_t nreg = 0;
	if (regions && fasim_read_bed(bed_path.c_str(), &reg, &nreg) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 2; }
	std::unique_ptr<fasim_region, void (*)(void*)> reg_owner(reg, fasim_free);
	Timers tm;
	const double t_start = now_s();
	std::vector<Rna> rnas;
	DnaReader reader;
	reader.upper = upper; reader.sticky_fields = accumulate;
	if (!reader.open(f1)) { fprintf(stderr, "fasim: cannot read DNA file %s\n", f1.c_str()); return 1; }
	if (!read_rnas(f2, rnas)) { fprintf(stderr, "fasim: cannot read RNA file %s\n", f2.c_str()); return 1; }
	if (trk.oligos) for (const Rna& r : rnas) if (r.seq.empty() || r.seq.size() > (size_t)FASIM_MAX_OLIGO) {
		fprintf(stderr, "fasim: --oligos: record '%s' in %s has %zu nt: an oligo has 1 to %d nt (longer queries: --sites without --oligos)\n", r.name.c_str(), f2.c_str(), r.seq.size(), FASIM_MAX_OLIGO);
		return 2;
	}
	for (const Rna& r : rnas) if (r.seq.empty()) { fprintf(stderr, "fasim: empty RNA record '%s' in %s\n", r.name.c_str(), f2.c_str()); return 1; }
	for (const Rna& r : rnas) if (r.seq.size() > (size_t)FASIM_MAX_QUERY) {
		fprintf(stderr, "fasim: RNA record '%s' in %s is %zu nt long, which exceeds the limit of %d nt: above it the reference's 16-bit "
			"stage-1 pass overruns its fixed workspace and its output is undefined\n", r.name.c_str(), f2.c_str(), r.seq.size(), FASIM_MAX_QUERY);
		return 1;
	}
	std::cout << "Searching triplexes using Fasim" << std::endl;
	for (const Rna& r : rnas) std::cout << r.name << std::endl;
	const std::string base = f1.substr(0, f1.size() >= 3 ? f1.size() - 3 : 0);
	// --regions index, one per lncRNA: <O>/<lncName>-<f1 minus 3 chars>.regions.tsv, one line per interval in BED order
	std::vector<std::vector<int64_t>> idx_segs(rnas.size(), std::vector<int64_t>((size_t)nreg, -1)), idx_trip = idx_segs;
	std::vector<std::vector<std::string>> idx_stem(rnas.size(), std::vector<std::string>((size_t)nreg));
	auto write_index = [&]() -> int {
		int bad = 0;
		for (size_t q = 0; q < rnas.size(); q++) {
			std::string t = "line\tname\tchrom\tstart\tend\tsegments\ttriplexes\tstem\n";
			for (int64_t k = 0; k < nreg; k++) {
				const fasim_region& g = reg[k];
				t += std::to_string(g.line) + "\t" + g.name + "\t" + g.chrom + "\t" + std::to_string(g.start) + "\t" + std::to_string(g.end) + "\t";
				if (idx_segs[q][(size_t)k] < 0) t += "NA\tNA\tNA\n";
				else t += std::to_string(idx_segs[q][(size_t)k]) + "\t" + std::to_string(idx_trip[q][(size_t)k]) + "\t" + idx_stem[q][(size_t)k] + "\n";
			}
			bad |= write_file(outdir + "/" + rnas[q].name + "-" + base + ".regions.tsv", t.data(), (int64_t)t.size());
		}
		return bad;
	};
	// --screen: per lncRNA and interval (--regions: BED order; --all-records: record order) the segments and the four peaks
	struct ScreenRow { int64_t line = 0, start = 0, end = 0, segs = -1; std::string name, chrom; };
	std::vector<ScreenRow> scr_rows((size_t)(trk.peaks && regions ? nreg : 0));
	for (int64_t k = 0; k < (int64_t)scr_rows.size(); k++) { ScreenRow& w = scr_rows[(size_t)k]; w.line = reg[k].line; w.start = reg[k].start; w.end = reg[k].end; w.name = reg[k].name; w.chrom = reg[k].chrom; }
	std::vector<std::vector<fasim_peak>> scr_peaks(trk.peaks ? rnas.size() : 0, std::vector<fasim_peak>(scr_rows.size() * 4));
	auto write_screen = [&]() -> int {
		int bad = 0;
		std::vector<fasim_region> rg(scr_rows.size()); std::vector<int64_t> sg(scr_rows.size());
		for (size_t k = 0; k < scr_rows.size(); k++) {
			const ScreenRow& w = scr_rows[k];
			rg[k].line = w.line; rg[k].start = w.start; rg[k].end = w.end; rg[k].chrom = w.chrom.c_str(); rg[k].name = w.name.c_str(); sg[k] = w.segs;
		}
		for (size_t q = 0; q < scr_peaks.size(); q++) {
			char* text = nullptr; int64_t len = 0;
			if (fasim_screen_tsv(rg.data(), sg.data(), scr_peaks[q].data(), (int64_t)rg.size(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			bad |= write_file(outdir + "/" + rnas[q].name + "-" + base + ".screen.tsv", text, len);
			fasim_free(text);
		}
		return bad;
	};
	// --tfo-profile: with --all-records / --regions one whole-set table per lncRNA, the maximum over the groups and records
	const bool tfo_set = (trk.tfo || trk.oligo_profile) && (all_records || regions);
	std::vector<fasim_tfo_profile*> tfo_acc(tfo_set ? rnas.size() : 0, nullptr);
	auto write_tfo = [&](const fasim_tfo_profile* t, const Rna& r, const std::string& path) -> int {
		// (no unit scanned: a table of zeros)
		std::vector<uint16_t> zeros(t ? 0 : r.seq.size() + 1, 0);
		fasim_tfo_profile z; z.m = (int32_t)r.seq.size(); z.units = z.saturated_units = 0;
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) z.v[c] = zeros.data();
		char* text = nullptr; int64_t len = 0;
		if (fasim_tfo_profile_tsv(t ? t : &z, r.seq.data(), r.name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		const int bad = write_file(path, text, len);
		fasim_free(text);
		return bad;
	};
	auto write_tfo_set = [&]() -> int {
		int bad = 0;
		for (size_t q = 0; q < tfo_acc.size(); q++) { bad |= write_tfo(tfo_acc[q], rnas[q], outdir + "/" + rnas[q].name + "-" + base + ".tfoprofile.tsv"); fasim_tfo_profile_free(tfo_acc[q]); tfo_acc[q] = nullptr; }
		return bad;
	};
	// --sites: a plain run writes <stem>-TFOsites-<V> per record; with --all-records / --regions one file per lncRNA,
	// <O>/<lnc>-<f1 stem>.sites-<V>.bed: one header line, then the records' sites in record / BED order, the record's name last
	const bool sites_set = sites && (all_records || regions);
	std::vector<std::map<int64_t, std::string>> sites_text(sites_set ? rnas.size() : 0);      // [lncRNA][record number or BED index]
	// --sites-align: beside every sites file the table of the sites' hits, <stem>-TFOsites-<V>-aligned or .sites-<V>.aligned.tsv
	std::vector<std::map<int64_t, std::string>> hits_text(sites_set && trk.hits() ? rnas.size() : 0);
	auto write_sites_set = [&]() -> int {
		int bad = 0;
		for (size_t q = 0; q < sites_text.size(); q++) {
			fasim_sites none; memset(&none, 0, sizeof none); none.min_value = trk.sites; none.max_gap = trk.sites_gap;
			char* text = nullptr; int64_t len = 0;
			if (fasim_sites_bed(&none, "", 1, rnas[q].name.c_str(), nullptr, 1, &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			std::string t(text, (size_t)len);
			fasim_free(text);
			for (const auto& kv : sites_text[q]) t += kv.second;
			bad |= write_file(outdir + "/" + rnas[q].name + "-" + base + ".sites-" + std::to_string(trk.sites) + ".bed", t.data(), (int64_t)t.size());
			if (!trk.hits()) continue;
			fasim_site_hits nohits; memset(&nohits, 0, sizeof nohits);
			if (fasim_site_hits_tsv(&none, &nohits, "", 1, rnas[q].name.c_str(), "", 1, &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			std::string h(text, (size_t)len);
			fasim_free(text);
			for (const auto& kv : hits_text[q]) h += kv.second;
			bad |= write_file(outdir + "/" + rnas[q].name + "-" + base + ".sites-" + std::to_string(trk.sites) + ".aligned.tsv", h.data(), (int64_t)h.size());
		}
		return bad;
	};
	// --potential-hist: the controls of every lncRNA; with --all-records / --regions / --oligos one table per lncRNA over everything
	// scanned, <O>/<lnc>-<f1 stem>.hist.tsv, summed over the groups; a plain run writes <stem>-TFOhist for its record
	std::vector<std::string> hist_ctl;
	if (trk.hist) {
		for (const Rna& r : rnas) for (int k = 1; k <= trk.hist_controls; k++) {
			std::string c(r.seq.size(), 'N');
			if ((trk.hist_dinuc ? fasim_shuffle_query_dinuc : fasim_shuffle_query)(r.seq.data(), (int32_t)r.seq.size(), trk.hist_seed, k, &c[0]) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			hist_ctl.push_back(std::move(c));
		}
		trk.hist_ctl = &hist_ctl;
	}
	const bool hist_set = trk.hist && (all_records || regions || trk.oligos);
	std::vector<fasim_hist*> hist_acc(hist_set && !trk.hist_sites ? rnas.size() + hist_ctl.size() : 0, nullptr);
	std::vector<fasim_site_counts*> counts_acc(hist_set && trk.hist_sites ? rnas.size() + hist_ctl.size() : 0, nullptr);
	// h: [lncRNAs] + [lncRNAs x K controls]; NULL entries (nothing scanned) stand for empty histograms
	auto write_hist = [&](fasim_hist* const* h, size_t q, const std::string& path) -> int {
		std::vector<int64_t> zeros(FASIM_HIST_BINS, 0);
		fasim_hist z; memset(&z, 0, sizeof z);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) z.n[c] = zeros.data();
		const size_t K = (size_t)trk.hist_controls;
		std::vector<const fasim_hist*> ctl(K);
		for (size_t k = 0; k < K; k++) { const fasim_hist* x = h[rnas.size() + q * K + k]; ctl[k] = x ? x : &z; }
		char* text = nullptr; int64_t len = 0;
		if (fasim_hist_tsv(h[q] ? h[q] : &z, ctl.data(), (int32_t)K, trk.hist_seed, trk.hist_fdr, rnas[q].name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		const int bad = write_file(path, text, len);
		fasim_free(text);
		return bad;
	};
	// --hist-sites: s as h above.  The hist table from the counts' n[][] (what --potential-hist alone writes), then the site counts
	auto write_counts = [&](fasim_site_counts* const* s, size_t q, const std::string& hist_path, const std::string& counts_path) -> int {
		std::vector<int64_t> zeros(FASIM_HIST_BINS, 0);
		fasim_site_counts z; memset(&z, 0, sizeof z);
		for (int c = 0; c < FASIM_TRACK_CLASSES; c++) { z.n[c] = zeros.data(); z.pairs[c] = zeros.data(); }
		const size_t K = (size_t)trk.hist_controls;
		std::vector<const fasim_site_counts*> all(1 + K);
		all[0] = s[q] ? s[q] : &z;
		for (size_t k = 0; k < K; k++) { const fasim_site_counts* x = s[rnas.size() + q * K + k]; all[1 + k] = x ? x : &z; }
		std::vector<fasim_hist> view(1 + K);
		std::vector<const fasim_hist*> vp(1 + K);
		for (size_t k = 0; k <= K; k++) {
			memset(&view[k], 0, sizeof view[k]);
			for (int c = 0; c < FASIM_TRACK_CLASSES; c++) view[k].n[c] = all[k]->n[c];
			view[k].positions = all[k]->positions; view[k].units = all[k]->units; view[k].saturated_units = all[k]->saturated_units;
			vp[k] = &view[k];
		}
		char* text = nullptr; int64_t len = 0;
		if (fasim_hist_tsv(vp[0], vp.data() + 1, (int32_t)K, trk.hist_seed, trk.hist_fdr, rnas[q].name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		int bad = write_file(hist_path, text, len);
		fasim_free(text);
		if (fasim_site_counts_tsv(all[0], all.data() + 1, (int32_t)K, trk.hist_seed, trk.hist_dinuc ? 1 : 0, trk.hist_fdr, rnas[q].name.c_str(), &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		bad |= write_file(counts_path, text, len);
		fasim_free(text);
		return bad;
	};
	auto write_hist_set = [&]() -> int {
		int bad = 0;
		for (size_t q = 0; q < rnas.size(); q++) {
			const std::string stem = outdir + "/" + rnas[q].name + "-" + base;
			bad |= trk.hist_sites ? write_counts(counts_acc.data(), q, stem + ".hist.tsv", stem + ".sitecounts.tsv") : write_hist(hist_acc.data(), q, stem + ".hist.tsv");
		}
		for (fasim_hist*& x : hist_acc) { fasim_hist_free(x); x = nullptr; }
		for (fasim_site_counts*& x : counts_acc) { fasim_site_counts_free(x); x = nullptr; }
		return bad;
	};
	// --oligos: the site lists of every oligo and record are kept for the panel table, <O>/<f2 stem>-<f1 stem>.oligos-<V>.tsv
	std::vector<std::vector<fasim_sites*>> panel_sites(trk.oligos ? rnas.size() : 0);
	auto write_panel = [&]() -> int {
		const size_t nq = rnas.size(), nr = nq ? panel_sites[0].size() : 0;
		std::vector<const char*> names(nq); std::vector<int32_t> lens(nq); std::vector<const fasim_sites*> flat;
		for (size_t q = 0; q < nq; q++) { names[q] = rnas[q].name.c_str(); lens[q] = (int32_t)rnas[q].seq.size(); flat.insert(flat.end(), panel_sites[q].begin(), panel_sites[q].end()); }
		char* text = nullptr; int64_t len = 0;
		if (fasim_oligo_panel_tsv(names.data(), lens.data(), (int32_t)nq, flat.data(), (int32_t)nr, &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		const int bad = write_file(outdir + "/" + f2.substr(0, f2.size() >= 3 ? f2.size() - 3 : 0) + "-" + base + ".oligos-" + std::to_string(trk.sites) + ".tsv", text, len);
		fasim_free(text);
		for (auto& v : panel_sites) { for (fasim_sites* x : v) fasim_sites_free(x); v.clear(); }
		return bad;
	};
	if (regions && nreg == 0) {
		if (tfo_set && write_tfo_set()) return 1;
		if (sites_set && write_sites_set()) return 1;
		if (trk.oligos && sites && write_panel()) return 1;
		if (hist_set && write_hist_set()) return 1;
		if (!screen_only && !trk.tfo_only && !trk.sites_only && !trk.hist_only && write_index()) return 1;
		if (trk.peaks && write_screen()) return 1;
		std::cout << "finished normally" << std::endl;
		return 0;
	}

	std::vector<fasim_engine*> engines;
	for (int d : devices) {
		fasim_engine* e = nullptr;
		if (fasim_engine_create(d, &e) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
		engines.push_back(e);
	}
	if (engines.size() > 1 && !getenv("FASIM_HOST_THREADS")) {
		// one process, several engines: every engine keeps six host threads per core of its share of the machine (at most the
		// single-engine default of 96; the host side of a batch is a burst that wants ~9 threads per batch in flight)
		const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
		const int per = std::max(16, (int)std::min(96u, 6 * (hc / (unsigned)engines.size())));
		for (fasim_engine* e : engines) fasim_set_option(e, "host_threads", per);
	}

	// file name: <O>/<species>-<lncName>-<f1 minus 3 chars>-TFOsorted (:123, 800-802); with --all-records the record's
	// chr is appended to the stem so that the records of a genome do not overwrite each other (--regions: <name>-...<chrom>)
	DnaRecord rec;
	size_t nrec = 0;
	int64_t total_nt = 0;
	std::deque<std::thread> pending;
	std::set<std::string> stems_seen;
	if (accumulate) {
		// B1: tmpDNA is never cleared, so record k holds records 1..k; all triplexes go into ONE list that is printed with
		// the first record's species / chr / start / length (main(), Fasim-LongTarget.cpp:133-166)
		std::vector<std::vector<fasim_result*>> per_rec;
		std::vector<long> starts;
		std::string first_species, first_chr, cumulative; long first_start = 0; int64_t first_len = 0;
		for (;;) {
			double t0 = now_s();
			if (!reader.next(rec)) break;
			tm.parse += now_s() - t0;
			cumulative += rec.seq;
			if (nrec == 0) { first_species = rec.species; first_chr = rec.chr; first_start = rec.start; first_len = (int64_t)cumulative.size(); }
			starts.push_back(rec.start);
			t0 = now_s();
			std::vector<fasim_result*> res;
			std::vector<fasim_track*> none;
			if (scan_record(engines, rnas, cumulative.data(), (int64_t)cumulative.size(), p, res, TrackOpt(), none)) return 1;
			tm.scan += now_s() - t0;
			total_nt += (int64_t)cumulative.size();
			per_rec.push_back(res);
			nrec++;
		}
		for (size_t q = 0; q < rnas.size() && nrec; q++) {
			std::vector<const fasim_triplex*> recs(nrec); std::vector<int64_t> counts(nrec), plens(nrec); std::vector<const char*> pools(nrec);
			for (size_t k = 0; k < nrec; k++) {
				fasim_result* r = per_rec[k][q];
				for (int64_t i = 0; i < r->count; i++) r->recs[i].genome_shift = (int32_t)(starts[k] - first_start);
				recs[k] = r->recs; counts[k] = r->count; pools[k] = r->pool; plens[k] = r->pool_len;
			}
			fasim_result* merged = nullptr;
			if (fasim_merge_results(recs.data(), counts.data(), pools.data(), plens.data(), (int32_t)nrec, &merged) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); return 1; }
			const std::string stem = outdir + "/" + first_species + "-" + rnas[q].name + "-" + base;
			if (write_outputs(merged, stem, first_chr, first_start, first_len, rnas[q].name, p, tail_flags, tm)) return 1;
			fasim_result_free(merged);
		}
		for (auto& v : per_rec) for (fasim_result* r : v) fasim_result_free(r);
	} else {
		// FASIM_RECORD_GROUP = G (--all-records, --regions): consecutive records are scanned together, one fasim_scan_records call
		// per group of about G segments; a record of >= G segments alone (a chromosome) is scanned as before.  0 = one scan per
		// record.  Default 5 120 = ten batches of 512 segments: one round of full batches for the ten workers of a scan.
		long group_segs = 5120;
		if (const char* g = getenv("FASIM_RECORD_GROUP")) group_segs = atol(g);
		// (--screen always takes the record-set call, a long record or FASIM_RECORD_GROUP=0 as a group of one)
		const bool grouped = (all_records || regions) && (group_segs > 0 || screen || sites || trk.hist || panel_extra);
		// grouped: the tails of thousands of records go to a pool of host threads instead of four threads in flight
		std::unique_ptr<TailPool> pool(grouped ? new TailPool(8) : nullptr);
		// one scanned record: a DNA record, or a BED interval (species = its name, start = its 1-based start; slot = its index)
		struct Unit { std::string species, chr; long start = 0; int64_t len = 0; size_t recno = 0; int64_t slot = -1; };
		// per record: --stats lines, output stem, tail + write on a background thread (the next record is read and scanned meanwhile)
		// the record's line of the screen tables
		auto screen_row = [&](const Unit& r, const fasim_peak* const* pk) {
			size_t row = (size_t)r.slot;
			if (!regions) {
				row = scr_rows.size();
				ScreenRow w; w.line = (int64_t)r.recno + 1; w.start = (int64_t)r.start - 1; w.end = w.start + r.len; w.name = r.species; w.chrom = r.chr;
				scr_rows.push_back(w);
				for (auto& v : scr_peaks) v.resize(scr_rows.size() * 4);
			}
			scr_rows[row].segs = fasim_segment_count(r.len, &p);
			for (size_t q = 0; q < rnas.size(); q++) for (int c = 0; c < 4; c++) scr_peaks[q][row * 4 + c] = pk[q][c];
		};
		auto emit = [&](const Unit& r, const std::vector<fasim_result*>& res, const std::vector<fasim_track*>& tracks, const fasim_peak* const* pk = nullptr, fasim_sites* const* st = nullptr, fasim_site_hits* const* ht = nullptr) {
			if (trk.oligo_screen) screen_row(r, pk);
			if (sites && st) {
				// the record's sites: its own file (a plain run), or its lines of the set's file
				for (size_t q = 0; q < rnas.size(); q++) {
					char* text = nullptr; int64_t len = 0;
					if (fasim_sites_bed(st[q], r.chr.c_str(), r.start, rnas[q].name.c_str(), sites_set ? r.species.c_str() : nullptr, sites_set ? 0 : 1, &text, &len) != FASIM_OK) {
						fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); g_out_failed = 1;
					} else if (sites_set) sites_text[q][r.slot >= 0 ? r.slot : (int64_t)r.recno].assign(text, (size_t)len);
					else if (write_file(outdir + "/" + r.species + "-" + rnas[q].name + "-" + base + "-TFOsites-" + std::to_string(trk.sites), text, len)) g_out_failed = 1;
					fasim_free(text);
					if (ht) {
						// the hits of those sites, line for line beside them
						text = nullptr;
						if (fasim_site_hits_tsv(st[q], ht[q], r.chr.c_str(), r.start, rnas[q].name.c_str(), sites_set ? r.species.c_str() : nullptr, sites_set ? 0 : 1, &text, &len) != FASIM_OK) {
							fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); g_out_failed = 1;
						} else if (sites_set) hits_text[q][r.slot >= 0 ? r.slot : (int64_t)r.recno].assign(text, (size_t)len);
						else if (write_file(outdir + "/" + r.species + "-" + rnas[q].name + "-" + base + "-TFOsites-" + std::to_string(trk.sites) + "-aligned", text, len)) g_out_failed = 1;
						fasim_free(text);
						fasim_site_hits_free(ht[q]);
					}
					if (trk.oligos) panel_sites[q].push_back(st[q]);
					else fasim_sites_free(st[q]);
				}
				if (trk.sites_only) return;
			}
			if (trk.hist_only) return;
			if (trk.oligos) return;      // (a panel has no triplex records)
			if (screen) {
				screen_row(r, pk);
				if (screen_only) return;
			}
			if (trk.tfo_only) return;
			for (size_t q = 0; q < rnas.size(); q++) {
				if (stats && res[q]) {
					const fasim_scan_stats& s = res[q]->stats;
					fprintf(stderr, "[fasim] record %zu (%s) x %s: %lld segments (%lld skipped), %lld units, %lld candidates, %lld align calls, %lld records\n",
						r.recno, r.chr.c_str(), rnas[q].name.c_str(), (long long)s.segments, (long long)s.segments_skipped, (long long)s.units,
						(long long)s.candidates, (long long)s.align_calls, (long long)res[q]->count);
				}
				const std::string name = r.species + "-" + rnas[q].name + "-" + base + (all_records || regions ? "." + r.chr : std::string());
				const std::string stem = outdir + "/" + name;
				const bool twice = !stems_seen.insert(stem).second;
				if (twice) fprintf(stderr, "fasim: warning: %s-TFOsorted is written twice (two lncRNAs or records of the same name): the later one wins\n", stem.c_str());
				fasim_result* x = res[q];
				int64_t* trip = nullptr;
				fasim_track* tk = tracks.empty() ? nullptr : tracks[q];
				const TrackOpt topt = trk;
				if (r.slot >= 0 && x) { idx_segs[q][(size_t)r.slot] = x->stats.segments; idx_stem[q][(size_t)r.slot] = name; trip = &idx_trip[q][(size_t)r.slot]; }
				const std::string chr = r.chr, lname = rnas[q].name; const long start = r.start; const int64_t dlen = r.len;
				auto job = [=, &tm, &p]() {
					Timers mine;
					int bad = x ? write_outputs(x, stem, chr, start, dlen, lname, p, tail_flags, mine, trip) : 0;
					fasim_result_free(x);
					if (tk) {
						// the potential track of the record: <stem>-TFOpotential-<BIN>
						char* text = nullptr; int64_t len = 0;
						if (fasim_track_bedgraph(tk, chr.c_str(), start, dlen, lname.c_str(), topt.min_value, &text, &len) != FASIM_OK) { fprintf(stderr, "fasim: %s\n", fasim_last_error(nullptr)); bad = 1; }
						else bad |= write_file(stem + "-TFOpotential-" + std::to_string(topt.bin), text, len);
						fasim_free(text);
						fasim_track_free(tk);
					}
					std::lock_guard<std::mutex> lk(g_out_mu);
					tm.tail += mine.tail; tm.write += mine.write; if (bad) g_out_failed = 1;
				};
				if (pool) {
					if (twice) pool->drain();         // the later one wins: the earlier file is complete before it is overwritten
					pool->add(job);
				} else {
					while (pending.size() >= 4) { pending.front().join(); pending.pop_front(); }
					pending.emplace_back(job);
				}
			}
		};
		// the pending group: its records' bytes packed side by side (a group may cross DNA records)
		std::vector<Unit> group;
		std::string gdna;
		std::vector<int64_t> goff, glen;
		int64_t group_nseg = 0;
		size_t ngroups = 0;
		auto flush = [&]() -> int {
			if (group.empty()) return 0;
			const double t0 = now_s();
			std::vector<std::vector<fasim_result*>> res;
			std::vector<std::vector<fasim_track*>> gtracks;
			std::vector<fasim_peak> gpeaks;
			std::vector<fasim_tfo_profile*> gprof;
			std::vector<std::vector<fasim_sites*>> gsites;
			std::vector<std::vector<fasim_site_hits*>> ghits;
			std::vector<fasim_hist*> ghist;
			std::vector<fasim_site_counts*> gcounts;
			if (scan_group(engines, rnas, gdna, goff, glen, p, res, trk, gtracks, gpeaks, trk.tfo || trk.oligo_profile ? &gprof : nullptr, sites ? &gsites : nullptr,
				sites && trk.hits() ? &ghits : nullptr, trk.hist && !trk.hist_sites ? &ghist : nullptr, trk.hist_sites ? &gcounts : nullptr)) return 1;
			if (trk.hist_sites && hist_set) { for (size_t k = 0; k < gcounts.size(); k++) { fasim_site_counts* t = gcounts[k]; gcounts[k] = nullptr; if (counts_fold(counts_acc[k], t)) return 1; } }
			else if (trk.hist_sites) {
				int bad = 0;
				for (size_t q = 0; q < rnas.size(); q++) {
					const std::string stem = outdir + "/" + group[0].species + "-" + rnas[q].name + "-" + base;
					bad |= write_counts(gcounts.data(), q, stem + "-TFOhist", stem + "-TFOsitecounts");
				}
				for (fasim_site_counts* x : gcounts) fasim_site_counts_free(x);
				if (bad) return 1;
			}
			else if (trk.hist && hist_set) { for (size_t k = 0; k < ghist.size(); k++) { fasim_hist* t = ghist[k]; ghist[k] = nullptr; if (hist_fold(hist_acc[k], t)) return 1; } }
			else if (trk.hist) {
				// a plain run: <stem>-TFOhist next to -TFOsorted
				int bad = 0;
				for (size_t q = 0; q < rnas.size(); q++) bad |= write_hist(ghist.data(), q, outdir + "/" + group[0].species + "-" + rnas[q].name + "-" + base + "-TFOhist");
				for (fasim_hist* x : ghist) fasim_hist_free(x);
				if (bad) return 1;
			}
			for (size_t q = 0; q < gprof.size(); q++) {
				fasim_tfo_profile* t = gprof[q]; gprof[q] = nullptr;
				if (tfo_set) { if (tfo_fold(tfo_acc[q], t)) return 1; continue; }
				// --oligos --oligo-profile on a plain run: <stem>-TFOprofile, the stem of the oligo's -TFOsites-<V> file
				const int bad = write_tfo(t, rnas[q], outdir + "/" + group[0].species + "-" + rnas[q].name + "-" + base + "-TFOprofile");
				fasim_tfo_profile_free(t);
				if (bad) return 1;
			}
			const double dt = now_s() - t0;
			tm.scan += dt;
			if (stats) fprintf(stderr, "[fasim] group %zu: %zu records, %lld segments, scan %.3f s\n", ngroups, group.size(), (long long)group_nseg, dt);
			std::vector<fasim_result*> one(rnas.size());
			std::vector<fasim_track*> onet(gtracks.size());
			std::vector<const fasim_peak*> onep(rnas.size(), nullptr);
			std::vector<fasim_sites*> ones(gsites.size());
			std::vector<fasim_site_hits*> oneh(ghits.size());
			for (size_t r = 0; r < group.size(); r++) {
				for (size_t q = 0; q < gsites.size(); q++) ones[q] = gsites[q][r];
				for (size_t q = 0; q < ghits.size(); q++) oneh[q] = ghits[q][r];
				for (size_t q = 0; q < rnas.size(); q++) one[q] = res[q][r];
				for (size_t q = 0; q < gtracks.size(); q++) onet[q] = gtracks[q][r];
				if (!gpeaks.empty()) for (size_t q = 0; q < rnas.size(); q++) onep[q] = gpeaks.data() + (q * group.size() + r) * 4;
				emit(group[r], one, onet, gpeaks.empty() ? nullptr : onep.data(), gsites.empty() ? nullptr : ones.data(), ghits.empty() ? nullptr : oneh.data());
				total_nt += group[r].len;
			}
			ngroups++; group.clear(); gdna.clear(); goff.clear(); glen.clear(); group_nseg = 0;
			return 0;
		};
		// one record: into the pending group if it is short, else scanned alone (the group is scanned first, keeping record order)
		auto add = [&](Unit u, const char* seq) -> int {
			if (grouped) {
				const int64_t ns = fasim_segment_count(u.len, &p);
				if (u.len > 0 && ns < group_segs) {
					group_nseg += ns;
					goff.push_back((int64_t)gdna.size()); glen.push_back(u.len);
					gdna.append(seq, (size_t)u.len);
					group.push_back(std::move(u));
					return group_nseg >= group_segs ? flush() : 0;
				}
				if (flush()) return 1;
				if (screen || sites || trk.hist || panel_extra) {
					// a group of one: only the record-set call gives the peaks / the sites
					group_nseg = fasim_segment_count(u.len, &p);
					goff.push_back(0); glen.push_back(u.len); gdna.assign(seq, (size_t)u.len); group.push_back(std::move(u));
					return flush();
				}
			}
			if (sites || trk.hist || panel_extra) {
				// a plain run: the record as a set of one (its records are those of fasim_scan_queries)
				group_nseg = fasim_segment_count(u.len, &p);
				goff.push_back(0); glen.push_back(u.len); gdna.assign(seq, (size_t)u.len); group.push_back(std::move(u));
				return flush();
			}
			const double t0 = now_s();
			std::vector<fasim_result*> res;
			std::vector<fasim_track*> tracks;
			std::vector<fasim_tfo_profile*> prof;
			if (scan_record(engines, rnas, seq, u.len, p, res, trk, tracks, trk.tfo ? &prof : nullptr)) return 1;
			for (size_t q = 0; q < prof.size(); q++) {
				fasim_tfo_profile* t = prof[q]; prof[q] = nullptr;
				if (tfo_set) { if (tfo_fold(tfo_acc[q], t)) return 1; continue; }
				// a plain run: <stem>-TFOprofile next to -TFOsorted
				const int bad = write_tfo(t, rnas[q], outdir + "/" + u.species + "-" + rnas[q].name + "-" + base + "-TFOprofile");
				fasim_tfo_profile_free(t);
				if (bad) return 1;
			}
			tm.scan += now_s() - t0;
			total_nt += u.len;
			emit(u, res, tracks);
			return 0;
		};
		// on an error the tails of earlier records still run on their threads: a joinable std::thread must not be destroyed
		auto stop = [&]() { for (std::thread& t : pending) t.join(); pool.reset(); return 1; };
		// --regions: the unmatched intervals of every chromosome, by start; an interval goes to the first DNA record (file order)
		// of its chromosome that holds it entirely.  held_start: a record held its start but ended before its end.
		std::map<std::string, std::multimap<int64_t, int64_t>> todo;
		std::set<std::string> chroms_seen;
		std::vector<char> held_start((size_t)nreg, 0);
		for (int64_t k = 0; k < nreg; k++) todo[reg[k].chrom].emplace(reg[k].start, k);
		for (;;) {
			double t0 = now_s();
			if (!reader.next(rec)) break;
			tm.parse += now_s() - t0;
			if (regions) {
				// '>species|chr|start-end' (a '|' in the first word; 1-based start, as the reference reads it) covers
				// [start - 1, start - 1 + len) of chr; any other header ('>chr1 AC:CM000663.2 ...', also with a '|' in its
				// description) names its chromosome by its first word and covers [0, len)
				std::string chrom = rec.chr; int64_t rs = (int64_t)rec.start - 1;
				const size_t w0 = rec.header.find_first_not_of("> \t\r");
				const std::string word = w0 == std::string::npos ? std::string() : rec.header.substr(w0, rec.header.find_first_of(" \t\r", w0) - w0);
				if (word.find('|') == std::string::npos) { chrom = word; rs = 0; }
				nrec++;
				chroms_seen.insert(chrom);
				auto it = todo.find(chrom);
				if (it == todo.end()) continue;
				const int64_t re = rs + (int64_t)rec.seq.size();
				std::vector<int64_t> mine;
				for (auto j = it->second.lower_bound(rs); j != it->second.end() && j->first < re; ) {
					if (reg[j->second].end <= re) { mine.push_back(j->second); j = it->second.erase(j); }
					else { held_start[(size_t)j->second] = 1; ++j; }
				}
				std::sort(mine.begin(), mine.end());   // BED order within the record
				for (int64_t k : mine) {
					const fasim_region& g = reg[k];
					Unit u; u.species = g.name; u.chr = g.chrom; u.start = (long)(g.start + 1); u.len = g.end - g.start; u.recno = (size_t)k; u.slot = k;
					if (add(std::move(u), rec.seq.data() + (g.start - rs))) return stop();
				}
				continue;
			}
			if (nrec > 0 && !all_records) {
				fprintf(stderr, "fasim: %s holds more than one record: only the first one was scanned (use --all-records; see DESIGN.md, B1)\n", f1.c_str());
				break;
			}
			Unit u; u.species = rec.species; u.chr = rec.chr; u.start = rec.start; u.len = (int64_t)rec.seq.size(); u.recno = nrec;
			if (add(std::move(u), rec.seq.data())) return stop();
			nrec++;
		}
		if (flush()) return stop();
		const double t_wait = now_s();
		for (std::thread& t : pending) t.join();
		pending.clear();
		if (pool) pool->drain();
		tm.tail_wait = now_s() - t_wait;
		if (g_out_failed) return 1;
		if (trk.peaks && write_screen()) return 1;
		if (tfo_set && write_tfo_set()) return 1;
		if (sites_set && write_sites_set()) return 1;
		if (trk.oligos && sites && write_panel()) return 1;
		if (hist_set && write_hist_set()) return 1;
		if (regions) {
			if (!screen_only && !trk.tfo_only && !trk.sites_only && !trk.hist_only && write_index()) return 1;
			std::vector<std::string> lost;
			for (const auto& c : todo) for (const auto& j : c.second) {
				const fasim_region& g = reg[j.second];
				const char* why = held_start[(size_t)j.second] ? "runs past the end of the DNA record that holds its start"
					: chroms_seen.count(g.chrom) ? "no DNA record of its chromosome holds it" : "no DNA record of its chromosome";
				char buf[512];
				snprintf(buf, sizeof buf, "fasim: BED line %lld (%s) %s:%lld-%lld: %s\n", (long long)g.line, g.name, g.chrom, (long long)g.start, (long long)g.end, why);
				lost.emplace_back(buf);
			}
			if (!lost.empty()) {
				// in BED order (the lines are numbered)
				std::vector<std::pair<int64_t, size_t>> order;
				size_t at = 0;
				for (const auto& c : todo) for (const auto& j : c.second) order.emplace_back(j.second, at++);
				std::sort(order.begin(), order.end());
				for (size_t k = 0; k < order.size() && k < 20; k++) fputs(lost[order[k].second].c_str(), stderr);
				if (lost.size() > 20) fprintf(stderr, "fasim: ... and %zu more\n", lost.size() - 20);
				fprintf(stderr, "fasim: %zu of %lld BED intervals lie in no DNA record of %s: their files were not written (NA in the index)\n",
					lost.size(), (long long)nreg, f1.c_str());
				for (fasim_engine* e : engines) fasim_engine_destroy(e);
				return 1;
			}
		}
	}
	if (nrec == 0) { fprintf(stderr, "fasim: no record in DNA file %s\n", f1.c_str()); return 1; }
	for (fasim_engine* e : engines) fasim_engine_destroy(e);
	if (stats) {
		const double total = now_s() - t_start;
		fprintf(stderr, "[fasim] end to end %.3f s: parse %.3f, scan %.3f, tail %.3f + write %.3f on background threads (%.3f s not hidden behind the next scan) (%zu DNA record(s), %lld nt, %zu lncRNA(s), %zu device shard(s)) = %.3f Mbp/s per lncRNA\n",
			total, tm.parse, tm.scan, tm.tail, tm.write, tm.tail_wait, nrec, (long long)total_nt, rnas.size(), engines.size(),
			(double)total_nt * (double)rnas.size() / total / 1e6);
	}
	std::cout << "finished normally" << std::endl;
	return 0;
}
