// fasim-longtarget_amd/csrc/engine.h -- internals of the host engine shared by its translation units (the C-ABI is
// include/fasim_hip.h; nothing here is exported).
//
// Data layout in HBM (one engine = one GPU):
//   dna        uint8[shard]                      the DNA shard, resident for the whole scan
//   tcodes     uint8[nunit][tstride]             target codes of every (segment x encoding) unit of the batch
//   colmax     uint8[nunit][tstride]             stage-2 column maxima (8-bit, as the reference's maxColumn)
//   q1/q2      uint8[m]                          query codes under the stage-1 / stage-2 alphabets
// Everything the kernels read is sized once per batch and reused; only small records cross PCIe.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <sched.h>
#include <malloc.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/fasim_hip.h"
#include "call_plan.h"
#include "device_types.h"
#include "host_post.h"
#include "kernels.h"

using namespace fasim;



inline thread_local std::string g_last_error;     // per thread: the CLI formats and writes outputs on background threads

// device (re)allocations since the process started: hipFree / hipMalloc synchronise the whole device, so a buffer that grows in
// the middle of a scan stalls every batch in flight (FASIM_PROFILE=1 prints the count per scan)
inline std::atomic<long> g_dev_reallocs{ 0 };
struct DevBuf {
	void* p = nullptr; size_t cap = 0;
	hipError_t ensure(size_t bytes) {
		if (bytes <= cap) return hipSuccess;
		g_dev_reallocs.fetch_add(1);
		if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
		size_t want = bytes + bytes / 4 + 256;
		hipError_t e = hipMalloc(&p, want);
		if (e != hipSuccess) { p = nullptr; return e; }
		cap = want;
		return hipSuccess;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
	template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// FASIM_PROFILE=1: wall-clock accumulators of the host phases, printed to stderr at the end of fasim_scan
struct HostProf {
	static constexpr int N = 32;
	double t[N] = { 0 }; const char* name[N] = { nullptr };
	bool on = false;
	std::mutex mu;
	void add(int i, const char* nm, double dt) { if (on) { std::lock_guard<std::mutex> g(mu); t[i] += dt; name[i] = nm; } }
	void dump() { if (!on) return; for (int i = 0; i < N; i++) if (name[i]) fprintf(stderr, "[fasim prof] %-60s %12.6f\n", name[i], t[i]); }
	void reset() { for (int i = 0; i < N; i++) { t[i] = 0; name[i] = nullptr; } }
};
inline HostProf g_prof;
static inline double thread_cpu_s() { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
struct CpuScope { int i; const char* nm; double t0; CpuScope(int i_, const char* n) : i(i_), nm(n), t0(g_prof.on ? thread_cpu_s() : 0.0) {} ~CpuScope() { if (g_prof.on) g_prof.add(i, nm, thread_cpu_s() - t0); } };
struct ProfScope { int i; const char* nm; double t0; ProfScope(int i_, const char* n) : i(i_), nm(n), t0(now_s()) {} ~ProfScope() { g_prof.add(i, nm, now_s() - t0); } };


struct fasim_engine {
	int device = 0;
	hipStream_t st = nullptr;
	std::string err;
	std::string rna;
	int m = 0;
	int snap_units = 0, snap_per_unit = 0;      // pipeline snapshots of the last main scan pass (units covered, snapshots per unit)
	ScoreLut lut1, lut2;
	DevBuf q1, q2, enc_lut, counter, dna, seg_start, seg_len, enc_ids, tcodes, colmax, probs, max_out, unit_len,
		stage1, hits, hits_total, hit_off, hit_cnt, thr, ends, bprobs, bout, scratch, colmax16, unit_ids, flags, stage1_in, hits2,
		fprobs, ftasks, fstream, fout, aout, cigpool, cigcount, forder, scratch2, boundary, fboundary, unit_hz,
		unit_first, hz_cols, hz_plan, hz_base, hz_items, snap, hz_state, hz_rows, hz_chunk, hz_src, hz_zero,   // chunked hazard re-run
		qsim, sim_min, sim_row, sim_ev, sim_cnt, sim_nodes,      // -F: query codes of the SIM alphabet, thresholds, strip row buffer, events, counters
		sim_req, sim_pairs, sim_used, sim_rounds, sim_col, sim_rowst, sim_state, sim_usedc, sim_debug, sim_nodes_in, sim_nodes_out, sim_out;   // -F re-sweeps: per-round requests, used pairs, DP state per column / row
	bool align_v1 = false;        // FASIM_ALIGN_V1=1: force the stripe-faithful kernels for stage 3
	std::vector<fasim_engine*> workers;   // extra engines on the same device: batches in flight concurrently
	// Gate for the two GPU-filling kernels (k_scan, k_align_fwd).  Without it the workers fall into lock step: all of them
	// launch a heavy kernel at once, the kernels share the GPU and end together, and then nothing heavy runs while all
	// workers do their latency-bound tail kernels and host work.  With at most `cap` heavy kernels in flight each one
	// runs at full speed and the workers stay staggered.
	struct HeavyGate { std::mutex m; std::condition_variable cv; int in_flight = 0; int cap = 3; };
	HeavyGate own_gate;
	HeavyGate* gate = nullptr;            // shared by the workers of one fasim_scan (points at the parent's own_gate)
	int host_threads_total = 1;
	int host_threads_share_total = 1;            // (workers) the scan's total, for the share of a worker near the end of a scan
	bool host_threads_explicit = false;          // FASIM_HOST_THREADS / option host_threads given: -F keeps to it too
	int scan_workers = 1;                        // worker engines of the scan in progress (they share the HBM)
	std::atomic<int>* sim_in_flight = nullptr;      // (set for the duration of a scan) -F: units in re-sweep launches right now, over all workers
	std::atomic<int>* active_workers = nullptr;  // (set for the duration of a scan) workers that still have batches: the host threads of
	                                             // those that have run out go to the bursts of the others
	int sim_threads = 1;                         // -F: host threads of this worker for the finish half (all cores shared by the batches in flight)
	int opt_workers = 0, opt_seg_batch = 0;      // fasim_set_option overrides (0 = default / environment)
	int opt_taper = -1, opt_gate = -1;           // (-1 = default / environment)
	int hz_chunks = -1, hz_snap = -1, hz_target = 0, hz_hot_w = 0;   // chunked hazard re-run: on/off, snapshots on/off (-1 = default / environment), chunk cost target, hot-column weight (0 = default)
	bool query_acgt = true;       // query holds only A,C,G,T: stage-1 and stage-2 scoring coincide on N-free segments
	bool scan_v1 = false;         // FASIM_SCAN_V1=1: force the stripe-faithful kernels for stages 1 and 2
	int host_threads = 1;
	// resident DNA record (fasim_load_dna)
	std::string dna_host;
	DevBuf dna_res;
	// streaming ingest (fasim_scan with a host buffer): pinned staging buffer of this worker's current batch slice
	void* pin_dna = nullptr; size_t pin_cap = 0;
	void* pin_sim = nullptr; size_t pin_sim_cap = 0;     // -F: node lists of a slice, both ways every launch
	// HIP-event timing of kernel launches on `st`
	struct Timed { hipEvent_t a, b; int family; };
	std::vector<Timed> timed;
	std::vector<hipEvent_t> ev_pool;
	double kernel_ms[FASIM_KERNEL_FAMILIES] = { 0 };
	int64_t kernel_launches[FASIM_KERNEL_FAMILIES] = { 0 };
	// banded stage 3 (band.hip): block maxima left by the last main k_scan pass of this engine, lists and column streams of the
	// tries selected per band class
	DevBuf ublk, btarget, bidx, bcounts, blist[3], bslots[3], bprev, lane_ub, fzones, fubslot, bdec, btab;
	int ublk_units = 0, ublk_blocks = 0;         // units covered by `ublk` (0: none), blocks per (unit, tile)
	int opt_band = -1;                           // option "band": 0 off, 1 on (-1 = default / environment FASIM_BAND)
	int opt_dp_f16 = -1;                         // option "dp_f16": packed-f16 k_scan and reverse pass, 0 = the integer kernels (-1 = default / environment FASIM_DP_F16)
	int opt_q2_past_cut = -1;                    // option "q2_past_cut": 1 = k_scan tracks Q2 taints to the end of every unit, 0 = up to a proven overflow cut (-1 = default / environment FASIM_Q2_PAST_CUT)
	int opt_finish_skip = -1;                    // option "finish_skip": 1 = the split finish leaves alignments the stability filter must drop without a CIGAR, 0 = k_finish_lds traces all, 2 = trace all and check the rule (-1 = default / environment FASIM_FINISH_SKIP)
	DevBuf fmask, flist, fmarks, seg_clean;      // the split finish: ballot masks per wave, the list of alignments to trace, mode 2's marks; per segment of the batch 1 = only ACGTN
	DevBuf unit_ovf;                             // [unit] != 0: the f16 k_scan saw a value outside its exact range
	DevBuf track, track_phase, track_sat;        // fasim_scan_track only: k_track's slices, its per-segment bin phase and saturation flags of the batch
	DevBuf track_peaks;                          // fasim_scan_records_track only: k_track's peak per slice and class
	DevBuf sites_counts, sites_offsets, sites_runs, sites_sat;   // fasim_scan_records_sites only: k_sites' run counts per (slice, class), their prefix sum, the runs and saturation flags of the batch
	DevBuf sa_q, sa_tcodes, sa_probs, sa_ends, sa_rows, sa_items, sa_dirs, sa_cigar, sa_ciglen;   // fasim_scan_records_sites_aligned only: query codes, the chunk's units, problems, end cells, row state of long queries, path items, direction bytes, CIGARs
	DevBuf hist, hist_zone, hist_zones, hist_sat;   // fasim_scan_records_hist only: k_hist's counters of the batch, its zone bounds per segment, the zone values and saturation flags
	DevBuf hist_pairs, hist_border;                 // fasim_scan_records_site_counts only (it uses the four above too): k_hist_pairs' pair counters and slice borders
	DevBuf vr_q, vr_dna, vr_alt, vr_probs, vr_tcodes, vr_rows, vr_touch, vr_out;   // the chunks of fasim_score_variants and fasim_score_haplotypes only: query codes, streamed window letters, ALT letters, problems, target codes, row state of long queries, k_touch's words, k_touch_reduce's words
	DevBuf vr_items, vr_dirs, vr_cigar, vr_paths;   // fasim_score_variants_aligned only: k_touch_path's items, direction bytes, CIGAR words and results
	DevBuf vr_hwins, vr_pieces, vr_ends;           // the same chunks: the windows, pieces and piece ends of k_hap_encode
	DevBuf mu_first, mu_groups, mu_snap, mu_cols, mu_pm;   // fasim_score_mutagenesis and fasim_score_deletions only: the units' column counts, the groups, the snapshots, the columns run and, for deletions, the column maxima.  Their launches use vr_q, vr_dna, vr_alt, vr_probs, vr_tcodes, vr_rows, vr_touch, vr_out, vr_hwins, vr_pieces and vr_ends as the chunks above do.
	int opt_sim_lds = -1;                        // option "sim_lds": -F re-sweeps always on the L2 variant (0) / the LDS variant where the state fits (1); -1 = by the units in flight
	int opt_site_short = -1;                     // option "site_short": 1 = the hits of oligo sites end on k_site_ends_short (default), 0 = on k_site_ends (-1 = default / environment FASIM_SITE_SHORT)
	int opt_site_chunk = 0;                      // option "site_chunk": problems per chunk of the hits phase where lower than the phase's own limit (0 = that limit)
	DevBuf oligo_q;                              // fasim_scan_oligos only: the panel's query codes, FASIM_MAX_OLIGO bytes per oligo
	DevBuf rowpart16;                            // fasim_scan_oligos_profile only: k_scan_short_rows' row maxima per (unit, stretch pair) of the batch (row_out and row_gfirst serve its fold)
	DevBuf rowmax16, row_out, row_gfirst, row_sat;   // fasim_scan_tfo_profile only: k_scan's row maxima of the batch, k_rowfold's groups, result and saturation flags
	int opt_numa = 1;                            // option "numa_affinity": pin the scan's host threads to the GPU's NUMA node (no-op on one node)
	// HBM-window variant of k_striped (queries whose stripes do not fit the LDS): its scratch, the forcing switch (option
	// "striped_window" / FASIM_STRIPED_WINDOW=1: every stripe-faithful launch takes it, for tests), problems run on it and its
	// HIP-event time since the counters were last taken
	DevBuf swin;
	bool striped_window = false;
	int64_t sw_probs = 0;
	double sw_ms = 0.0;
};



inline int fail(fasim_engine* e, int code, const char* fmt, ...)
{
	char buf[1024];
	va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
	g_last_error = buf;
	if (e) e->err = buf;
	return code;
}

// a malloc'ed, NUL-terminated copy of `s`, as the text functions of the C-ABI return it
inline int text_out(const std::string& s, char** text, int64_t* text_len)
{
	char* buf = (char*)malloc(s.size() + 1);
	if (!buf) return fail(nullptr, FASIM_E_NOMEM, "out of memory");
	memcpy(buf, s.data(), s.size()); buf[s.size()] = 0;
	*text = buf; *text_len = (int64_t)s.size();
	return FASIM_OK;
}

#define HIPOK(call) do { hipError_t _e = (call); if (_e != hipSuccess) return fail(E, FASIM_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); } while (0)

// stage-2/3 alphabet (ssw_cpp.cpp:13-26): A,a,U,u -> 0 ; C,c -> 1 ; G,g -> 2 ; T,t -> 3 ; else 4
inline uint8_t code2(char c) { switch (c) { case 'A': case 'a': case 'U': case 'u': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; } }
// SIM (-F) alphabet: upper-case ACGT; the engine's and the oracle's choice is that every other letter (U, N, IUPAC codes, lower
// case) is a mismatch (-4) with everything.  That is NOT the reference's behaviour: its table `long V[128][128]` is a local of SIM()
// (sim.h:419) of which only the 16 ACGT x ACGT entries are ever written (sim.h:470-473), so for any other pair it reads
// uninitialised stack memory and its output is undefined (DESIGN sections 7 and 9)
inline uint8_t sim_code(char c) { switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; } }
// stage-1 alphabet (stats.h:201-228, 306-334): U == T, everything outside ACGTU is N
inline uint8_t code1(char c) { switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 4; } }

inline ScoreLut make_lut(bool stage1)
{
	// row t, entry q (4 bits): score(t,q) + BIAS ; entry 5 = pad row = score 0
	ScoreLut L;
	for (int t = 0; t < 5; t++) {
		uint32_t w = 0;
		for (int q = 0; q < 5; q++) {
			int s;
			if (stage1) s = (t == 4 || q == 4) ? -1 : (t == q ? 5 : -4);      // npam: N row all -1 (stats.h:227-228)
			else s = (t == q && t < 4) ? 5 : -4;                              // ssw_cpp.cpp:28-53
			w |= (uint32_t)(s + BIAS) << (4 * q);
		}
		w |= (uint32_t)BIAS << 20;
		L.row[t] = w;
	}
	return L;
}

// ---- HIP-event timing ----------------------------------------------------------------------------
inline hipEvent_t get_event(fasim_engine* E)
{
	if (!E->ev_pool.empty()) { hipEvent_t e = E->ev_pool.back(); E->ev_pool.pop_back(); return e; }
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) != hipSuccess) return nullptr;
	return e;
}
// TimedScope family: FASIM_KERNEL_FAMILIES index, plus TIMED_WINDOW for a k_striped launch on the HBM-window variant
constexpr int TIMED_FAMILY_MASK = 0xff, TIMED_WINDOW = 0x100;
struct TimedScope {
	fasim_engine* E; hipEvent_t a = nullptr, b = nullptr; int family;
	hipStream_t s;
	TimedScope(fasim_engine* e, int fam, hipStream_t stream = nullptr) : E(e), family(fam), s(stream ? stream : e->st) { a = get_event(E); b = get_event(E); if (a) (void)hipEventRecord(a, s); }
	~TimedScope() { if (a && b) { (void)hipEventRecord(b, s); E->timed.push_back({ a, b, family }); } }
};
// call after a stream synchronisation
inline void drain_timed(fasim_engine* E)
{
	for (auto& t : E->timed) {
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
			const int fam = t.family & TIMED_FAMILY_MASK;
			E->kernel_ms[fam] += ms; E->kernel_launches[fam]++;
			if (t.family & TIMED_WINDOW) E->sw_ms += ms;
		}
		E->ev_pool.push_back(t.a); E->ev_pool.push_back(t.b);
	}
	E->timed.clear();
}

// ---- a batch of units whose target codes are resident on the device ------------------------------
struct UnitBatch {
	int nunit = 0;
	int tstride = 0;
	std::vector<int> unit_len;      // columns per unit
};

// H2D copy without the trailing synchronisation: the caller keeps `src` alive until its next stream synchronisation
inline int upload_async(fasim_engine* E, DevBuf& b, const void* src, size_t bytes)
{
	HIPOK(b.ensure(bytes ? bytes : 1));
	if (bytes) HIPOK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, E->st));
	return FASIM_OK;
}

inline int upload(fasim_engine* E, DevBuf& b, const void* src, size_t bytes)
{
	HIPOK(b.ensure(bytes ? bytes : 1));
	// sources are short-lived pageable host vectors: make the copy complete before returning
	if (bytes) { HIPOK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, E->st)); HIPOK(hipStreamSynchronize(E->st)); }
	return FASIM_OK;
}

inline std::vector<StripedProb> whole_unit_probs(const UnitBatch& B, int m, const std::vector<int>* subset)
{
	std::vector<StripedProb> v;
	const int n = subset ? (int)subset->size() : B.nunit;
	v.reserve(n);
	for (int k = 0; k < n; k++) {
		const int u = subset ? (*subset)[k] : k;
		StripedProb p; p.tbase = (int64_t)u * B.tstride; p.t0 = 0; p.ref_len = B.unit_len[u]; p.q_len = m; p.unit = u; p.aux = 0; p.pad = 0;
		v.push_back(p);
	}
	return v;
}


// ---- stages 1+2 through the fused systolic kernel (scan.hip) -----------------------------------------
struct ScanOut {
	std::vector<int32_t> stage1, thr, hit_off, hit_cnt, flags;
	std::vector<uint32_t> hits;
};


struct GateScope {
	fasim_engine::HeavyGate* g;
	explicit GateScope(fasim_engine* E) : g(E->gate)
	{
		if (!g) return;
		std::unique_lock<std::mutex> lk(g->m);
		g->cv.wait(lk, [&] { return g->in_flight < g->cap; });
		g->in_flight++;
	}
	void release()
	{
		if (!g) return;
		{ std::lock_guard<std::mutex> lk(g->m); g->in_flight--; }
		g->cv.notify_one();
		g = nullptr;
	}
	~GateScope() { release(); }
};

// cores this process may really use: scheduler affinity, capped by the cgroup CPU quota when there is one
// (std::thread::hardware_concurrency() reports the whole host on a shared GPU node)
inline int usable_cores()
{
	int n = (int)std::max(1u, std::thread::hardware_concurrency());
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof set, &set) == 0) { const int a = CPU_COUNT(&set); if (a > 0) n = std::min(n, a); }
	if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
		char q[64] = { 0 }; long long period = 0;
		if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) { const long long c = atoll(q) / period; if (c >= 1) n = (int)std::min<long long>(n, c); }
		fclose(f);
	}
	return std::max(1, n);
}

// Banded stage 3 (band.hip): classes usable for the current query; 0 = off (FASIM_BAND=0 / option band = 0, stripe-faithful
// modes, queries the band kernel does not hold)
// option band / FASIM_BAND: 0 off, 1 on (default), 2 = bands from k_scan's block maxima only, no reverse passes (for measurements)
inline int band_mode(const fasim_engine* E)
{
	static const int env = [] { const char* e = getenv("FASIM_BAND"); return e ? atoi(e) : 1; }();
	return E->opt_band >= 0 ? E->opt_band : env;
}
// option site_short / FASIM_SITE_SHORT: 1 (default) = fasim_scan_oligos_aligned finds the end and start cells with k_site_ends_short,
// 0 = with k_site_ends (the A/B arm and the fallback; the results are the same)
inline bool site_short_enabled(const fasim_engine* E)
{
	static const int env = [] { const char* e = getenv("FASIM_SITE_SHORT"); return e ? atoi(e) : 1; }();
	return (E->opt_site_short >= 0 ? E->opt_site_short : env) != 0;
}
// option dp_f16 / FASIM_DP_F16: 1 (default) = k_scan's main pass and the reverse pass of stage 3 run their packed-f16 variants
// (dp_f16.h); 0 = the integer kernels.  The records are the same either way.
inline bool dp_f16_mode(const fasim_engine* E)
{
	static const int env = [] { const char* e = getenv("FASIM_DP_F16"); return e ? atoi(e) : 1; }();
	return (E->opt_dp_f16 >= 0 ? E->opt_dp_f16 : env) != 0;
}
// option q2_past_cut / FASIM_Q2_PAST_CUT: 0 (default) = the k_scan passes of run_scan_v2 stop the Q2 taint tracking of a unit once a
// clean block maximum >= 251 has proven its overflow cut (scan.hip); 1 = they track to the end of the unit.  The records, the
// hazard units and every statistic are the same either way: only bit 0 of column maxima behind the cut differs.
inline bool q2_past_cut_mode(const fasim_engine* E)
{
	static const int env = [] { const char* e = getenv("FASIM_Q2_PAST_CUT"); return e ? atoi(e) : 0; }();
	return (E->opt_q2_past_cut >= 0 ? E->opt_q2_past_cut : env) != 0;
}
// option finish_skip / FASIM_FINISH_SKIP: 1 (default) = the scan's finish runs k_finish_rev / k_finish_trace and leaves the alignments
// that doomed.h proves to fail the stability filter without a CIGAR; 0 = k_finish_lds traces every alignment; 2 = every alignment is
// traced and the rule is checked against the full conversion (stats finish_skip_violations).  The records are the same in all three.
inline int finish_skip_mode(const fasim_engine* E)
{
	static const int env = [] { const char* e = getenv("FASIM_FINISH_SKIP"); return e ? atoi(e) : 1; }();
	const int v = E->opt_finish_skip >= 0 ? E->opt_finish_skip : env;
	return v < 0 || v > 2 ? 1 : v;
}
inline int band_mask(const fasim_engine* E)
{
	if (!band_mode(E) || E->align_v1 || E->scan_v1) return 0;
	return band_classes(E->m);
}

// CPUs of the NUMA node the GPU hangs on (local_cpulist of its PCI device), intersected with what this thread may use.  false:
// unknown, or no restriction (single-node machine): nothing to pin.
inline bool gpu_local_cpus(int device, cpu_set_t* out)
{
	char bus[64] = { 0 };
	if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return false; }
	for (char* c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
	char path[160]; snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
	FILE* f = fopen(path, "r");
	if (!f) return false;
	char list[1024] = { 0 };
	const bool ok = fgets(list, sizeof list, f) != nullptr;
	fclose(f);
	if (!ok) return false;
	cpu_set_t local; CPU_ZERO(&local);
	for (const char* p = list; *p && *p != '\n'; ) {
		char* e = nullptr;
		const long a = strtol(p, &e, 10);
		if (e == p) break;
		long b = a; p = e;
		if (*p == '-') { b = strtol(p + 1, &e, 10); p = e; }
		for (long k = a; k <= b && k < CPU_SETSIZE; k++) if (k >= 0) CPU_SET((int)k, &local);
		if (*p == ',') p++;
	}
	cpu_set_t allowed;
	if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return false;
	CPU_AND(out, &local, &allowed);
	const int n = CPU_COUNT(out);
	return n > 0 && n < CPU_COUNT(&allowed);
}
// Pins the calling thread (and the worker / host threads it starts, which inherit the mask) to the GPU's NUMA node for the
// duration of a scan: on an 8-GPU node every rank / every --devices engine then keeps its host side next to its own GPU
// instead of wandering over both sockets.  Option numa_affinity = 0 leaves the affinity alone.
struct AffinityScope {
	cpu_set_t saved; bool active = false;
	AffinityScope(int device, bool enabled) {
		cpu_set_t local;
		if (!enabled || sched_getaffinity(0, sizeof saved, &saved) != 0 || !gpu_local_cpus(device, &local)) return;
		active = sched_setaffinity(0, sizeof local, &local) == 0;
	}
	~AffinityScope() { if (active) (void)sched_setaffinity(0, sizeof saved, &saved); }
};

// FASIM_HAZARD_CHUNKS=0: whole-unit re-run of the hazard units (the round-1 path); FASIM_HAZARD_SNAP=0: the checkpoint pass
// runs every hazard unit from column 0 instead of from the main pass's pipeline snapshots (both for measurements)
// (options hazard_chunks / hazard_snapshots override the environment)
inline bool hazard_chunks_enabled(const fasim_engine* E) { static const bool v = [] { const char* e = getenv("FASIM_HAZARD_CHUNKS"); return e ? atoi(e) != 0 : true; }(); return E->hz_chunks >= 0 ? E->hz_chunks != 0 : v; }
// Snapshots are OFF by default since round 3: they cost 67 KB of HBM writes per unit (2.3 x the algorithmic traffic of k_scan, 1.4 GB
// per batch in flight) for the 0.8 % of the units that become hazard units, and buy 7 ms of a batch's latency that ten batches in flight
// hide anyway (2.18 vs 2.21 s per 50 Mb step, inside the run-to-run noise: profiles/r03_ab_snapshots.txt).
inline bool hazard_snapshots_enabled(const fasim_engine* E) { static const bool v = [] { const char* e = getenv("FASIM_HAZARD_SNAP"); return e ? atoi(e) != 0 : false; }(); return E->hz_snap >= 0 ? E->hz_snap != 0 : v; }


// ---- the batched body of LongTarget() ---------------------------------------------------------------
// One batch of segments [b0, b1) on one worker engine (own stream and buffers): encode, scan, candidates, window
// alignments, triplex records.  Several batches run concurrently on different workers (fasim_scan below).
// What one batch leaves after its scan phase (stages 1+2) and what its stage 3 needs: host-side hit lists and segment
// tables, plus a pointer to the target codes that stay resident on the owner engine.  Stage 3 is separable by unit range
// (stage3_range), so near the end of a scan a batch publishes its stage 3 as sub-tasks that idle workers take over.
// (the segment table of a call, SegTable, and the cuts into batches: call_plan.h)

// ---- products of a scan: what a call takes from k_scan's column and row maxima besides the hits -----------------------------------
struct BatchCtx;
// One product of one call (potential tracks, the lncRNA's profile, sites, histogram), shared by the call's workers.  Behind the main
// pass of a batch run_scan_v2 runs fold() of every product of the call; the worker runs merge() after the batch's next stream
// synchronisation.  fasim_scan_oligos (engine_oligos.cpp) does the same per oligo behind k_scan_short.
struct ScanProduct {
	bool only = false;                           // no hits, no hazard re-run, no stage 3, no records
	std::unique_ptr<std::mutex[]> mu;            // [query]: merge() works under the query's
	virtual ~ScanProduct() = default;
	virtual bool wants_rowmax() const { return false; }      // k_scan's main pass and its integer re-run leave their row maxima in E->rowmax16
	virtual bool merges_empty() const { return false; }      // a batch whose segments are all skipped is merged too
	virtual const char* needs_scan() const = 0;              // the refusal of a batch that did not go through the systolic scan kernel
	// the batch's host preparation, the launches over E->colmax16 (E->rowmax16) and the copies into C's vectors for query q; the copies
	// complete at the next synchronisation of E->st
	virtual int fold(fasim_engine* E, BatchCtx& C, int q) const = 0;
	// C's vectors of a finished scan phase, segments [b0, b1) of the call's table, into the call's arrays of query q (may throw std::bad_alloc)
	virtual void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) = 0;
};
// the products of one call in fold and merge order; empty: a plain scan
typedef std::vector<ScanProduct*> ScanProducts;
inline bool any_only(const ScanProducts& ps) { for (const ScanProduct* x : ps) if (x->only) return true; return false; }
inline bool any_rowmax(const ScanProducts& ps) { for (const ScanProduct* x : ps) if (x->wants_rowmax()) return true; return false; }

// ---- potential tracks (fasim_scan_track, track.hip) ------------------------------------------------------------------------------
// One call: the record's arrays (those of the fasim_track objects the call returns), which the workers fold their batches' slices
// into as soon as a batch's scan phase ends; a bin that two batches touch (overlapping segments) is merged under the query's mutex.
struct TrackReq : ScanProduct {
	int bin = 1;                                 // bin == 0: peaks only, no arrays
	int nrec = 1;                                // records of the call (fasim_scan_track: 1); o = query * nrec + record below
	std::vector<int64_t> nbins;                  // [record]
	std::vector<uint16_t*> v;                    // [o * 4 + class][nbins[record]] (empty with bin == 0)
	fasim_peak* peaks = nullptr;                 // [o * 4 + class], preset to (0, -1, -1), or NULL: no peaks (fasim_scan_records_track)
	std::vector<int64_t> sat;                    // [o]: units with a saturated column maximum
	const char* needs_scan() const override { return "potential tracks need the systolic scan kernel"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
	void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) override;
};
inline fasim_track* track_alloc(int64_t nbins, int32_t bin)
{
	fasim_track* t = (fasim_track*)calloc(1, sizeof(fasim_track));
	if (!t) return nullptr;
	t->nbins = nbins; t->bin = bin;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
		t->v[c] = (uint16_t*)calloc((size_t)std::max<int64_t>(1, nbins), sizeof(uint16_t));
		if (!t->v[c]) { fasim_track_free(t); return nullptr; }
	}
	return t;
}

// ---- per-base profile of the lncRNA (fasim_scan_tfo_profile, rowfold.hip) ---------------------------------------------------------
// One call: the arrays of the fasim_tfo_profile objects the call returns, per o = query * nrec + record (per_record) or per query;
// the workers fold their batches' groups into them under the query's mutex as soon as a batch's scan phase ends.
struct TfoReq : ScanProduct {
	bool per_record = false;
	int nrec = 1;
	std::vector<int32_t> m;                      // [query]: rows of the result
	std::vector<uint16_t*> v;                    // [o * 4 + class][m[query]]
	std::vector<int64_t> units, sat;             // [o]: units folded in, units with a saturated row maximum
	bool wants_rowmax() const override { return true; }
	const char* needs_scan() const override { return "the lncRNA's profile needs the systolic scan kernel"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
	void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) override;
};
// The profile of an oligo of a panel (fasim_scan_oligos_profile, engine_oligos.cpp): the same arrays and the same merge, but the rows
// are the oligo's own m[q] -- the engine's query is not involved -- and fold() runs k_rowfold_parts over E->rowpart16, which
// panel_batch has k_scan_short_rows fill.  No value reaches saturation (5 * 112 = 560).
struct OligoTfoReq : TfoReq {
	const char* needs_scan() const override { return "an oligo's profile needs k_scan_short"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
};
inline fasim_tfo_profile* tfo_profile_alloc(int32_t m)
{
	fasim_tfo_profile* t = (fasim_tfo_profile*)calloc(1, sizeof(fasim_tfo_profile));
	if (!t) return nullptr;
	t->m = m;
	for (int c = 0; c < FASIM_TRACK_CLASSES; c++) {
		t->v[c] = (uint16_t*)calloc((size_t)std::max<int32_t>(1, m), sizeof(uint16_t));
		if (!t->v[c]) { fasim_tfo_profile_free(t); return nullptr; }
	}
	return t;
}

// ---- sites above a fixed potential (fasim_scan_records_sites, sites.hip) -------------------------------------------------------------
// One run as the workers keep it: record positions, the encoding itself
struct HostRun { int64_t start, end, pos; int32_t value, enc, cls; };
// One call: per o = query * nrec + record the runs of the record's slices as k_sites cut them, appended by the workers under the
// query's mutex as soon as a batch's scan phase ends; sorted, united and joined when the call ends (sites_build in fasim_scan_records_sites, engine.cpp)
struct SitesReq : ScanProduct {
	int min_value = 1, max_gap = 0;
	int nrec = 1;
	std::vector<std::vector<HostRun>> runs;      // [o]
	std::vector<int64_t> sat;                    // [o]: units with a saturated column maximum
	const char* needs_scan() const override { return "sites need the systolic scan kernel"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
	void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) override;
};
// The second phase of fasim_scan_records_sites_aligned (engine_site_align.cpp, site_align.hip): after the call's sites are final,
// every site of (query q, record r) gets its hit.  The phase runs chunk by chunk on the engine's own stream and buffers (sa_*).
struct SiteAlignReq {
	const char* dna = nullptr;                   // host DNA of the call (the caller's buffer or the resident copy)
	const int64_t* rec_off = nullptr; const int64_t* rec_len = nullptr; int nrec = 1;
	int64_t seg_first = 0, seg_count = -1;       // the call's range of the global segment list
	fasim_params p;
	std::vector<std::string> queries;
	fasim_sites* const* sites = nullptr;         // [query * nrec + record], final
	fasim_site_hits** hits = nullptr;            // [query * nrec + record], filled by the phase
	// fasim_scan_oligos_aligned (section 18): every query has at most SCAN_SHORT_MAX nt and the ends launch is k_site_ends_short --
	// a problem is a lane, not a workgroup, so a chunk takes 262 144 problems and no row state.  false: everything as it was
	bool short_query = false;
};
int run_site_align(fasim_engine* E, SiteAlignReq& R);
void site_hits_free(fasim_site_hits* h);
// One hit on its way into a fasim_site_hits.  aligned: cigar and strings are there; otherwise cigar_len = -1 and the hit counts as
// unaligned, except an `empty` one (a slot of fasim_score_variants_aligned without a value): cigar_len = 0, not counted
struct HitOut {
	HostTriplex t;
	int32_t i0 = -1, i1 = -1, j0 = -1, j1 = -1;
	std::vector<uint32_t> cigar;
	bool aligned = false, empty = false;
};
void hit_clear(HitOut& H, int enc);                            // the numbers of a hit that has no alignment (yet): zeros, seg -1
fasim_site_hits* pack_hits(const std::vector<HitOut>& v);      // NULL: out of memory
// The path k_site_path / k_touch_path returned between the cells H already carries, as a hit: `len` CIGAR words, last operation first,
// over the n letters `seg` from `origin` of their record.  Where convert_triplex gives no record, H stays unaligned as it was.
void path_hit(HitOut& H, const uint32_t* cig, int len, int value, const std::string& rna, const char* seg, int n, int enc, long origin, const fasim_params& pc, int seg_id);
// One launch of path items (SitePathItem, TouchPathItem): items[a .. end) get their dir_off and cig_off, up to the item that would
// take the direction bytes past dir_cap or the CIGAR words past cig_cap (the first always fits); dims(item) = its {rows, columns}.
struct LaunchCut { size_t end; int64_t dir_total, cig_total; int max_rows; };
template <class Item, class Dims>
LaunchCut cut_launch(std::vector<Item>& items, size_t a, int64_t dir_cap, int64_t cig_cap, Dims dims)
{
	LaunchCut c = { a, 0, 0, 1 };
	for (; c.end < items.size(); c.end++) {
		Item& I = items[c.end];
		const std::pair<int64_t, int64_t> d = dims(I);
		if (c.end > a && (c.dir_total + d.first * d.second > dir_cap || c.cig_total + I.cig_cap > cig_cap)) break;
		I.dir_off = c.dir_total; I.cig_off = (int32_t)c.cig_total;
		c.dir_total += d.first * d.second; c.cig_total += I.cig_cap; c.max_rows = std::max(c.max_rows, (int)d.first);
	}
	return c;
}

// ---- histogram of the potential (fasim_scan_records_hist, hist.hip, engine_hist.cpp) ---------------------------------------------
// One side of the overlap of two neighbouring segments of a record, as the values of that segment alone: boundary b of a record is
// the overlap of its segments b and b + 1, side 0 the tail zone of segment b, side 1 the head zone of segment b + 1.  An empty `v`
// stands for zeros (a segment that same_seq() skips).
struct HistSide { int32_t len = 0; std::vector<uint16_t> v; /* [4][len] */ };
struct HistEdgeKey {
	int32_t rec; int64_t boundary; int32_t side;
	bool operator<(const HistEdgeKey& o) const { return rec != o.rec ? rec < o.rec : boundary != o.boundary ? boundary < o.boundary : side < o.side; }
};
// One call: per query the counters of the fasim_hist the call returns, and the zone sides that wait for their partner (the other
// batch, or the merge of the shards when the partner lies outside the call's range).  The workers add under the query's mutex.
struct HistReq : ScanProduct {
	int64_t step = 0, overlap = 0;               // cutLength - overlapLength, overlapLength
	std::vector<int64_t> rec_nseg;               // [record]: segments of the whole record
	std::vector<int32_t> qtop;                   // [query]: largest value the query can reach (the copy back stops there)
	std::vector<int64_t*> n;                     // [query * 4 + class][HIST_BINS]
	std::vector<int64_t> positions, units, sat;  // [query]
	std::vector<std::map<HistEdgeKey, HistSide>> open;      // [query]: sides whose partner has not arrived
	std::vector<std::vector<std::pair<HistEdgeKey, HistSide>>> pending;   // [query]: sides whose partner lies outside the call's range
	bool merges_empty() const override { return true; }      // (the positions of skipped segments lie in bin 0)
	const char* needs_scan() const override { return "the histogram of the potential needs the systolic scan kernel"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
	void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) override;
};

// ---- sites per threshold (fasim_scan_records_site_counts, hist_pairs.hip, engine_site_counts.cpp) -----------
// One side of a boundary as a HistSide, with the values of the position next to the zone on the interior side of its segment
// (fasim_site_counts_edge: nb, link).  An empty `v` stands for zeros.
struct PairSide { int32_t len = 0, link = 0; uint16_t nb[4] = { 0, 0, 0, 0 }; std::vector<uint16_t> v; /* [4][len] */ };
// The counters of one query and the sides that have no partner yet.  Every side is counted alone when it comes in and the two of a
// boundary are re-counted as their maximum when they meet: a batch in a call and a shard in a merge are the same thing.
struct PairBook {
	int64_t* n[4] = { nullptr, nullptr, nullptr, nullptr }; int64_t* pairs[4] = { nullptr, nullptr, nullptr, nullptr };
	int64_t positions = 0, npairs = 0;
	std::map<HistEdgeKey, PairSide> open;
};
struct SiteCountsReq : ScanProduct {
	int64_t step = 0, overlap = 0;               // cutLength - overlapLength, overlapLength
	std::vector<int64_t> rec_nseg;               // [record]: segments of the whole record
	std::vector<int32_t> qtop;                   // [query]: largest value the query can reach (the copy back stops there)
	std::vector<PairBook> book;                  // [query]
	std::vector<int64_t> units, sat;             // [query]
	bool merges_empty() const override { return true; }      // (the positions of skipped segments lie in bin 0)
	const char* needs_scan() const override { return "site counts need the systolic scan kernel"; }
	int fold(fasim_engine* E, BatchCtx& C, int q) const override;
	void merge(const BatchCtx& C, const SegTable& T, int64_t b0, int64_t b1, int q) override;
};

struct BatchCtx {
	UnitBatch B;
	// what the products' folds leave of this batch (ScanProduct::fold): `folded` once run_scan_v2 has run them
	bool folded = false;
	TrackTable tab; int track_nchunk = 0;              // class table of the enabled encodings, TRACK_CHUNK slices per segment (batch_encode)
	std::vector<uint32_t> hist; std::vector<uint16_t> hist_zones; std::vector<uint8_t> hist_sat; std::vector<int32_t> hist_zone;      // fasim_scan_records_hist: k_hist's counters, zones and zone bounds
	int hist_zstride = 0, hist_top = 0;
	std::vector<uint32_t> hist_pairs; std::vector<uint16_t> hist_border;      // fasim_scan_records_site_counts (with the four above): k_hist_pairs' pair counters and slice borders
	std::vector<uint32_t> site_counts; std::vector<SiteRun> site_runs; std::vector<uint8_t> site_sat;      // fasim_scan_records_sites: k_sites' runs
	std::vector<uint16_t> rowfold; std::vector<uint8_t> row_sat; std::vector<int32_t> row_gfirst;      // fasim_scan_tfo_profile: k_rowfold's groups
	std::vector<uint16_t> track; std::vector<uint8_t> track_sat;      // fasim_scan_track: k_track's slices
	std::vector<TrackPeak> track_peaks;                               // fasim_scan_records_track: its peaks
	// the folds' large vectors, once merged: the batch's stage 3 follows
	void release_folded() { std::vector<uint16_t>().swap(rowfold); std::vector<uint16_t>().swap(track); std::vector<SiteRun>().swap(site_runs); std::vector<uint16_t>().swap(hist_zones); }
	int tstride = 0, nenc = 0, nseg = 0;
	int64_t step = 0;
	// per kept segment of the batch: device start (relative to the batch's DNA on the device), length, index within its record
	// (dna_start = sidx * step, triplex `seg`), offset in the host DNA buffer, record
	std::vector<int32_t> sstart, slen; std::vector<int64_t> sidx, soff; std::vector<int32_t> srec;
	std::vector<int32_t> ucand, ualign;                 // per unit: candidates and window tries of stage 3 (per-record stats)
	std::vector<int32_t> hoff, hcnt, thr; std::vector<uint32_t> hits;
	std::vector<char> seg_acgtn;
	const uint8_t* dna_dev = nullptr;                   // the batch's DNA on the device: E->seg_start counts from here (batch_encode)
	const char* dna = nullptr; const fasim_params* p = nullptr; const std::vector<int>* encs = nullptr;
	std::vector<std::vector<HostTriplex>> per_unit;     // [unit]: records of the unit after fastSIM's own filter
	bool stage3_done = false;                           // -F: the whole batch was finished in the scan phase
};

// ---- what the folds of the products share (engine_stage2.cpp, engine_hist.cpp) -----------------------------------------------------
// the front half's arguments of a column fold over batch C, its saturation flags in `sat`
inline void class_fold_fill(ClassFoldLaunch& L, const fasim_engine* E, const BatchCtx& C, const DevBuf& sat)
{
	L.colmax16 = E->colmax16.as<uint16_t>(); L.seg_len = E->seg_len.as<int32_t>();
	L.nseg = C.nseg; L.nenc = C.nenc; L.tstride = C.B.tstride; L.nchunk = C.track_nchunk; L.tab = C.tab; L.sat = sat.as<uint8_t>();
}
// The zones of k_hist and k_hist_pairs: head-zone end and tail-zone begin of segment i (length L) of a record of `nseg` segments cut
// with step = cutLength - overlapLength.  The one place that states which positions two segments share
inline void hist_zone_bounds(int64_t step, int64_t overlap, int64_t i, int32_t L, int64_t nseg, int32_t* head, int32_t* tail)
{
	*head = i > 0 ? (int32_t)std::min<int64_t>(overlap, L) : 0;
	*tail = i + 1 < nseg ? (int32_t)step : L;      // (a segment with a successor is longer than the step)
}
// the zone bounds of the batch's kept segments into C.hist_zone ([nseg][2], what both kernels read); returns the longest zone
inline int hist_zone_table(BatchCtx& C, int64_t step, int64_t overlap, const std::vector<int64_t>& rec_nseg)
{
	C.hist_zone.resize((size_t)C.nseg * 2);
	int zmax = 0;
	for (int s = 0; s < C.nseg; s++) {
		int32_t h, t;
		hist_zone_bounds(step, overlap, C.sidx[(size_t)s], C.slen[(size_t)s], rec_nseg[(size_t)C.srec[(size_t)s]], &h, &t);
		C.hist_zone[(size_t)2 * s] = h; C.hist_zone[(size_t)2 * s + 1] = t;
		zmax = std::max(zmax, std::max(h, C.slen[(size_t)s] - t));
	}
	return zmax;
}
// a fold's saturation flags, one per unit: ensured and zeroed on the stream ahead of the launch ...
inline int sat_begin(fasim_engine* E, DevBuf& dev, size_t nu)
{
	HIPOK(dev.ensure(nu));
	HIPOK(hipMemsetAsync(dev.p, 0, nu, E->st));
	return FASIM_OK;
}
// ... and their copy into the batch's vector (sized by the caller) queued behind it
inline int sat_end(fasim_engine* E, const DevBuf& dev, std::vector<uint8_t>& host)
{
	HIPOK(hipMemcpyAsync(host.data(), dev.p, host.size(), hipMemcpyDeviceToHost, E->st));
	return FASIM_OK;
}
// a batch's flags onto the counts per o = q * nrec + record of the unit's segment
inline void sat_add(std::vector<int64_t>& sat, const std::vector<uint8_t>& flags, const BatchCtx& C, int q, int nrec)
{
	for (size_t u = 0; u < flags.size(); u++) sat[(size_t)q * (size_t)nrec + (size_t)C.srec[u / (size_t)C.nenc]] += flags[u];
}

// ---- internals shared by the engine's translation units (engine.cpp: C-ABI; engine_stage2.cpp: stages 1+2; engine_stage3.cpp:
//      stage 3; engine_scan.cpp: batches, workers, result packing) ------------------------------------------------------------
struct WindowProb { int unit, t0, len; };
inline const uint8_t* tcv(const fasim_engine* E) { return E->tcodes.as<uint8_t>(); }
// input of the reverse pass (band.hip, align.hip): per window the lengths of the candidate's next three tries (zone tags of the
// reversed stream) and the candidate's slot in E->lane_ub
struct FwdZones { std::vector<uint32_t> zones; std::vector<int32_t> slot; };

int run_striped(fasim_engine* E, StripedMode mode, bool word, const std::vector<StripedProb>& probs, bool stage1, const uint8_t* tcodes, int max_qlen);
int prep_striped_window(fasim_engine* E, StripedMode mode, bool word, StripedLaunch& L, bool* used);
int run_stage1(fasim_engine* E, const UnitBatch& B, std::vector<int>& score, int64_t* word_reruns);
int run_stage2(fasim_engine* E, const UnitBatch& B);
// the products' folds run behind the main pass (and its integer re-run) of batch C, for query q; 1: the query does not fit the kernel
int run_scan_v2(fasim_engine* E, BatchCtx& C, const std::vector<char>& unit_needs_stage1, ScanOut& out, fasim_scan_stats* st, const ScanProducts& products, int q);
int load_raw_targets(fasim_engine* E, const char* targets, const int64_t* offsets, const int32_t* lens, int nprob, bool stage1, UnitBatch& B);
int need_query(fasim_engine* E);
int run_align(fasim_engine* E, const UnitBatch& B, const std::vector<WindowProb>& W, std::vector<AlignResult>& out, std::vector<uint32_t>& cigars, fasim_scan_stats* stats);
// path (may be null): per window, what produced its alignment (0 nothing aligned, 1-4 the finish tier, 5 the stripe-faithful replay)
int run_align_v2(fasim_engine* E, const UnitBatch& B, const std::vector<WindowProb>& W, std::vector<AlignResult>& out, std::vector<uint32_t>& cigars, fasim_scan_stats* stats,
	std::vector<int32_t>* path = nullptr);
int stage3_range(fasim_engine* E, BatchCtx& C, int ua, int ub, fasim_scan_stats& st);
int scan_batch(fasim_engine* E, const char* dna, const SegTable& T, const uint8_t* dna_dev, int64_t b0, int64_t b1,
	const fasim_params& p, const std::vector<int>& encs, int tstride, BatchCtx& C, fasim_scan_stats& st, const ScanProducts& products, int q);
// the head of a batch (segments kept, DNA staged, k_encode, class table), shared by scan_batch and fasim_scan_oligos (engine_oligos.cpp)
int batch_encode(fasim_engine* E, const char* dna, const SegTable& T, const uint8_t* dna_dev, int64_t b0, int64_t b1,
	const fasim_params& p, const std::vector<int>& encs, int tstride, BatchCtx& C, fasim_scan_stats& st, int64_t m);
// engine_hist.cpp: the request of a call and its results
bool hist_req_init(HistReq& hr, fasim_hist** out_hists, int nquery, const int32_t* qlens, const int64_t* rec_len, int nrec, const fasim_params& p, bool only);
int hist_req_finish(fasim_engine* E, HistReq& hr, fasim_hist** out_hists, int nquery);
// engine_site_counts.cpp: the same for the site counts
bool site_counts_req_init(SiteCountsReq& sr, fasim_site_counts** outs, int nquery, const int32_t* qlens, const int64_t* rec_len, int nrec, const fasim_params& p, bool only);
int site_counts_req_finish(fasim_engine* E, SiteCountsReq& sr, fasim_site_counts** outs, int nquery);

// ---- the frame of a call (engine.cpp; the pure part is call_plan.h; DESIGN.md "the frame of a call") ----------------------------------
// The record set of a call as its entry point got it, resolved: `dna` NULL stands for the resident buffer, and an entry point that
// takes "dna, rec_off and rec_len all NULL, nrec 1" as the whole resident buffer gets that record from here (whole_off, whole_len).
struct RecordSet {
	const char* dna = nullptr; const int64_t* rec_off = nullptr; const int64_t* rec_len = nullptr; int32_t nrec = 0;
	bool resident = false;
	int64_t whole_off = 0, whole_len = 0;
	RecordSet() = default;
	RecordSet(const RecordSet&) = delete;
	RecordSet& operator=(const RecordSet&) = delete;
	const char* host(const fasim_engine* E) const { return dna ? dna : E->dna_host.data(); }
};
// The record-set check of every entry point, in two steps, because the callers' own checks (cutLength, queries, ...) have always
// stood between them.  record_set_open: the whole-resident-buffer record (whole_ok), nrec, the arrays.  record_set_bounds: resident
// DNA present, no empty record, every record inside the (resident) buffer and at most 2^31-1 nt.
int record_set_open(fasim_engine* E, const char* dna, const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, bool whole_ok, RecordSet& rs);
int record_set_bounds(fasim_engine* E, const RecordSet& rs);
// the refusals of a call that scores variants or intervals, before its entries are looked at (engine_variants.cpp)
int check_variant_call(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna, const int64_t* rec_off,
	const int64_t* rec_len, int32_t nrec, int32_t flank, const fasim_params* pp, RecordSet& rs);
// both steps around the checks of the lncRNA entry points (pp, nq, cutLength / overlapLength, the queries or the engine's own)
int check_records_args(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, const fasim_params* pp, bool whole_ok, RecordSet& rs);
int check_track_source(fasim_engine* E, const int32_t* rna_lens, int32_t nq, const fasim_params* pp, const char* what = "potential tracks");
// the call's option / environment: worker engines wanted (FASIM_WORKERS, option workers) and a fixed batch (FASIM_SEG_BATCH, option
// seg_batch; 0: none given)
int workers_wanted(const fasim_engine* E);
int64_t seg_batch_given(const fasim_engine* E);
// ws = E and its first wanted - 1 worker engines on the same device, created where missing
int worker_set(fasim_engine* E, int wanted, std::vector<fasim_engine*>& ws);
// worker w of E's call before its first item: the encodings up, the kernel timers drained and zeroed
int worker_begin(fasim_engine* E, fasim_engine* w, const std::vector<int>& encs);
// ... after each item: the stream synchronised, the timers into the item's stats and zeroed
void worker_item_end(fasim_engine* w, fasim_scan_stats& st);
// ... and when all have joined: the first worker's error wins, with its text on E
int workers_result(fasim_engine* E, const std::vector<fasim_engine*>& ws, const std::vector<int>& wrc);
// The results a call needs but its caller did not ask for: `outs` is the caller's array or one of `n` that dies with this object.
struct OwnResults {
	std::vector<fasim_result*> own;
	fasim_result** outs;
	OwnResults(fasim_result** wanted, size_t n) : own(wanted ? 0 : n, nullptr), outs(wanted ? wanted : own.data()) {}
	~OwnResults() { for (fasim_result* r : own) fasim_result_free(r); }
	OwnResults(const OwnResults&) = delete;
	OwnResults& operator=(const OwnResults&) = delete;
};
// a TrackReq over nquery x nrec outputs: with bin >= 1 out_tracks[o] is allocated (all released and NULL again on failure) and tr.v
// points into them; bin 0: peaks only
int track_req_init(fasim_engine* E, TrackReq& tr, int32_t bin, bool only, int nquery, const int64_t* rec_len, int nrec, fasim_track** out_tracks, fasim_peak* peaks);
void tracks_drop(fasim_track** out_tracks, size_t nout);
// a SitesReq over nquery x nrec outputs, and its runs as site lists: out_sites[o] with units(o) units (all released and NULL again on failure)
void sites_req_init(SitesReq& sr, int32_t min_value, int32_t max_gap, bool only, int nquery, int nrec);
int sites_req_finish(fasim_engine* E, const SitesReq& sr, fasim_sites** out_sites, const std::function<int64_t(size_t)>& units);
void sites_drop(fasim_sites** out_sites, size_t nout);
// fasim_scan_records_sites; `rs` hands the resolved record set to fasim_scan_records_sites_aligned (engine_site_align.cpp)
int scan_records_sites(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int32_t nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int32_t nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	int32_t min_value, int32_t max_gap, fasim_result** out_results, fasim_sites** out_sites, fasim_scan_stats* totals, RecordSet& rs);
int sim_forward_units(fasim_engine* E, const uint8_t* tcodes_dev, int tstride, const int32_t* unit_len_dev, const int32_t* unit_len_host,
	int first, int nunit, const int64_t* mins, std::atomic<int>* ready, std::vector<std::vector<fasim_sim_node>>& lists);
int sim_resweep_rounds(fasim_engine* E, const uint8_t* tcodes_dev, int tstride, const int32_t* unit_len_dev, const int32_t* unit_len_host,
	int first, int cnt, SimUnit* const* units, int nthreads, fasim_scan_stats* st);
int pack_result(fasim_engine* E, std::vector<HostTriplex>& all, const fasim_scan_stats& st, fasim_result** out);
int scan_core(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int nq, const char* dna, int64_t dna_len,
	int64_t seg_first, int64_t seg_count, const fasim_params* pp, fasim_result** outs, const ScanProducts& products = {});
// the class tables of k_track / k_rowfold: the enabled encodings by group = class + 4 * reversed
TrackTable class_table(const std::vector<int>& encs);
// fasim_scan_records after its argument checks: records [rec_off[r], rec_off[r] + rec_len[r]) of `dna` (NULL: the resident
// buffer); outs[q * nrec + r], totals[q] (may be NULL)
int scan_records_core(fasim_engine* E, const char* const* rnas, const int32_t* rna_lens, int nq, const char* dna,
	const int64_t* rec_off, const int64_t* rec_len, int nrec, int64_t seg_first, int64_t seg_count, const fasim_params* pp,
	fasim_result** outs, fasim_scan_stats* totals, const ScanProducts& products = {});
