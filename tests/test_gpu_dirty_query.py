"""lncRNA queries with U, lower case, N and IUPAC letters on the GPU.  fasim_set_query keeps three encodings of the query: the
stage-1 alphabet (U == T, every letter outside ACGTU is N and scores -1), the stage-2/3 alphabet (U is read as A, the reference's
quirk; every other letter scores -4) and the -F alphabet (upper-case ACGT only).  A query with such letters also clears
query_acgt, so that every unit takes the separate stage-1 pass of run_scan_v2.  The inputs are helpers.dirty_case (generated); the
expected values are the reference's (tests/golden/dirtyq_*, probe_dirty40.rsp.gz, `make_golden.py dirtyq`), which
test_oracle_golden.py ties to the oracle and whose input conditions it checks.  All comparisons are exact.  GPU only."""
import os
import struct

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

SYSTOLIC = {100: False, 700: True, 1300: True, 4000: True}


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def cases(golden_dir):
    """m -> query, DNA and the reference's units, each made once and left unchanged"""
    cache = {}

    def get(m):
        if m not in cache:
            rna, dna = helpers.dirty_case(m)
            _, units = helpers.parse_scan(helpers.gunzip(os.path.join(golden_dir, f"dirtyq_{m}.scan.gz")))
            cache[m] = {"rna": rna, "dna": dna, "units": units, "base": None}
        return cache[m]

    return get


def _scan(mod, rna, dna, p=None, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_query(rna)
    r = e.scan(dna, p or mod.default_params(cLength=20))     # cLength == ntMin: LongTarget's tail filter == fastSIM's
    e.close()
    return r


def _base(mod, c):
    if c["base"] is None:
        c["base"] = _scan(mod, c["rna"], c["dna"])
    return c["base"]


def _clean(m):
    """The query of the case before its letters were made untidy: upper-case ACGT."""
    return synth.random_rna(m, helpers.DIRTY_SEEDS[m])


# ---- 1. raw kernels ------------------------------------------------------------------------------------------------------------------
def test_raw_kernels_against_reference_probe(mod, golden_dir):
    """calc_score_once (stage-1 alphabet), ssw_pre_align (stage-2 alphabet) and ssw_align of a 900-nt untidy query, batched and one
    call at a time, against the reference probe's recorded answers; where the compiled reference travelled with the repository
    (oracle/_ref), the live probe must still give those answers."""
    q, targets, wins, reqs = helpers.probe_dirty_vectors()
    rsp = helpers.gunzip(os.path.join(golden_dir, "probe_dirty40.rsp.gz")).decode().splitlines()
    assert len(rsp) == len(reqs)
    if helpers.have_ref_probe():
        assert helpers.ref_batch(reqs) == rsp
    e = mod.Engine(0)
    e.set_query(q)
    cols, s1 = e.pre_align_batch(targets)
    als = e.align_batch(wins)
    for k in range(40):
        exp_s1 = int(rsp[3 * k].split(" ")[1])
        exp_cols = [int(x) for x in rsp[3 * k + 1].split(" ")[2:]]
        assert s1[k] == exp_s1 and e.calc_score_once(targets[k]) == exp_s1, k
        assert cols[k] == exp_cols and e.ssw_pre_align(targets[k]) == exp_cols, k
        g = rsp[3 * k + 2].split(" ")
        for a in (als[k], e.ssw_align(wins[k])):
            if int(g[1]) == 0:
                assert a.sw_score == 0, k
            else:
                assert (a.sw_score, a.ref_begin, a.ref_end, a.query_begin, a.query_end) == tuple(int(x) for x in g[1:6]), k
                assert (a.cigar_string() or "*") == g[6], k
    e.close()


# ---- 2. the scan, four query classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", helpers.DIRTY_LENGTHS)
def test_scan_equals_the_reference(mod, cases, golden_dir, m):
    """Every triplex of the reference bit for bit, the candidate and unit counts, and -TFOsorted at -lg 30 (1 300 and 4 000 rows)."""
    c = cases(m)
    res = _base(mod, c)
    st = res.stats
    print(f"m {m}: units {st['units']}, candidates {st['candidates']}, stage1_word_reruns {st['stage1_word_reruns']}, hazard_units {st['hazard_units']}, "
          f"k_scan launches {st['kernel_launches'][0]}, band_tries {st['band_tries']}, dp_f16_reruns {st['dp_f16_reruns']}")
    assert st["units"] == len(c["units"]) == 144
    assert st["candidates"] == sum(u["ncand"] for u in c["units"])
    assert res.triplexes() == helpers.expected_triplexes(c["units"])
    if SYSTOLIC[m]:
        # run_scan_v2 adds to stage1_word_reruns the units it sends through the separate k_scan pass with the stage-1 query codes
        # (and units whose doubled 16-bit lanes saturate, of which these cases hold none): with an untidy query that is every unit
        assert st["kernel_launches"][0] > 0
        assert st["stage1_word_reruns"] == st["units"]
    else:
        # 100 rows: stage 1 runs on the stripe-faithful kernels for every unit anyway; there the stat counts the units whose byte
        # pass overflowed and was run again in 16 bits, which says nothing about the query's letters (kernel_launches[0] counts the one
        # k_scan launch that is refused for a query this short)
        assert st["band_tries"] == 0
    assert st["hazard_units"] >= helpers.DIRTY_Q2_UNITS.get(m, 0)
    if m >= 1300:
        p = mod.default_params(cLength=30)
        _, chro, start = mod.parse_dna_header(helpers.DIRTY_DNA_HEADER)
        text = mod.tfosorted(_scan(mod, c["rna"], c["dna"], p), chro, start, p)
        assert text == open(os.path.join(golden_dir, f"dirtyq_{m}.TFOsorted"), "rb").read()


# ---- 3. every organisation of the work gives the same records -----------------------------------------------------------------------
SWITCHES = ({"dp_f16": 0}, {"dp_f16": 1}, {"band": 0}, {"band": 1}, {"band": 2}, {"striped_window": 1}, {"hazard_chunks": 0},
            {"hazard_chunks": 1, "hazard_chunk_cols": 64})


@pytest.mark.parametrize("m", [1300, 4000])
def test_organisations_agree(mod, cases, monkeypatch, m):
    """The integer and the f16 DP, stage 3 without bands, with them and without reverse passes, the HBM-window variant of k_striped,
    whole-unit and chunked hazard re-runs, and the stripe-faithful kernels everywhere (FASIM_SCAN_V1 / FASIM_ALIGN_V1): the records,
    the pool and the candidates of the default scan.  (4 000 rows: two tiles, so the chunked re-run has no snapshots to start from.)"""
    c = cases(m)
    base = _base(mod, c)
    assert base.count > 0 and base.stats["hazard_units"] > 0 and base.stats["band_tries"] > 0
    for opts in SWITCHES:
        r = _scan(mod, c["rna"], c["dna"], **opts)
        assert (r.recs, r.pool) == (base.recs, base.pool), (m, opts)
        assert r.stats["candidates"] == base.stats["candidates"], (m, opts)
        if opts == {"band": 0}:
            assert r.stats["band_tries"] == 0
    monkeypatch.setenv("FASIM_SCAN_V1", "1")
    monkeypatch.setenv("FASIM_ALIGN_V1", "1")
    r = _scan(mod, c["rna"], c["dna"])
    assert (r.recs, r.pool) == (base.recs, base.pool), (m, "V1")
    assert r.stats["candidates"] == base.stats["candidates"] and r.stats["kernel_launches"][0] == 0


# ---- 4. query_acgt belongs to the query, not to the engine ---------------------------------------------------------------------------
def test_untidy_and_clean_queries_on_one_engine(mod, cases):
    """scan_queries([clean, untidy, clean]) equals three scans; a clean query set after an untidy one scans like on a fresh engine
    (no separate stage-1 pass: the DNA holds no N); and a record set scanned with the untidy query equals its single scans, one
    segment per batch and with the default batches."""
    c = cases(1300)
    dirty, dna = c["rna"], c["dna"]
    clean = _clean(1300)
    p = mod.default_params(cLength=20)
    alone = {clean: _scan(mod, clean, dna)}
    alone[dirty] = _base(mod, c)
    assert alone[clean].recs != alone[dirty].recs
    assert alone[clean].stats["stage1_word_reruns"] == 0 and alone[dirty].stats["stage1_word_reruns"] == 144
    e = mod.Engine(0)
    batch = e.scan_queries([clean, dirty, clean], dna, p)
    for r, q in zip(batch, (clean, dirty, clean)):
        assert (r.recs, r.pool) == (alone[q].recs, alone[q].pool)
        for k in ("units", "candidates", "stage1_word_reruns"):
            assert r.stats[k] == alone[q].stats[k], k
    e.set_query(dirty)
    e.set_query(clean)
    r = e.scan(dna, p)
    assert (r.recs, r.pool) == (alone[clean].recs, alone[clean].pool) and r.stats["stage1_word_reruns"] == 0
    e.set_query(dirty)
    r = e.scan(dna, p)
    assert (r.recs, r.pool) == (alone[dirty].recs, alone[dirty].pool) and r.stats["stage1_word_reruns"] == 144
    records = [dna[:3100], dna[3000:8200], dna[8100:]]
    single = [e.scan(d, p) for d in records]
    assert sum(s.count for s in single) > 0
    for seg_batch in (1, 0):
        if seg_batch:
            e.set_option("seg_batch", seg_batch)
        else:
            e.close()
            e = mod.Engine(0)
            e.set_query(dirty)
        got = e.scan_records(records, p)
        for g, s in zip(got, single):
            assert (g.recs, g.pool) == (s.recs, s.pool), seg_batch
            assert g.stats["candidates"] == s.stats["candidates"]
    e.close()


# ---- 6. -F (classic SIM) --------------------------------------------------------------------------------------------------------------
def _simscan_triplexes(text, c_length):
    """X lines of `simscan` with LongTarget()'s tail filter (as test_gpu_parity._simscan_expected), as scan() tuples"""
    out, seg, enc = [], 0, 0
    for line in text.decode().splitlines():
        f = line.split(" ")
        if f[0] == "V":
            seg, enc = int(f[1]), int(f[2])
        elif f[0] == "X":
            ident = struct.unpack("<f", struct.pack("<I", int(f[10], 16)))[0]
            tri = struct.unpack("<f", struct.pack("<I", int(f[11], 16)))[0]
            if float(int(f[9])) >= 0.0 and ident >= 60.0 and tri >= 1.0 and int(f[8]) >= c_length:
                out.append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]),
                            int(f[10], 16), int(f[11], 16), f[12].encode(), f[13].encode(), seg, enc))
    return out


@pytest.mark.parametrize("m", [100, 700])
def test_classic_sim_equals_the_oracle(mod, oracle_build, tmp_path, m):
    """-F with an untidy query against the ORACLE's simscan, not the reference: the reference's SIM() fills its score table for
    ACGT x ACGT only and reads uninitialised stack memory for every other pair, so its output is undefined
    there.  The engine and the oracle both score such a pair as a mismatch (-4); lower-case letters and U are such letters."""
    rna_fa, dna_fa, rna, dna = helpers.dirty_case_files(tmp_path, m)
    exp = _simscan_triplexes(helpers.oracle_cli(oracle_build, "simscan", rna_fa, dna_fa, "-threads", "16"), 20)
    res = _scan(mod, rna, dna, mod.default_params(classicSim=1, cLength=20))
    rows = helpers.dirty_rows(rna)
    over = {k: sum(helpers.triplex_rows_overlap(x, r) for x in exp) for k, r in rows.items()}
    print(f"m {m}: {len(exp)} triplexes under -F, over untidy rows {over}")
    assert len(exp) > 0 and res.triplexes() == exp
    assert res.stats["kernel_launches"][7] > 0, "k_sim_forward must have run"
