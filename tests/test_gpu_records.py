"""Record sets (fasim_scan_records / Engine.scan_records / `fasim --all-records` groups): many short DNA records scanned in
shared batches give, record by record, exactly what a scan of that record alone gives.  GPU only."""
import os
import subprocess

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

NREC, NENC = 532, 48
SEVEN = ("segments", "segments_skipped", "units", "candidates", "align_calls", "logical_cells", "cells_stage2")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def engine(mod):
    e = mod.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def peaks(golden_dir):
    return helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))


def _rna(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _same(a, b):
    return a.recs == b.recs and a.pool == b.pool


_PEAKS = {}


def _peak_results(mod, engine, golden_dir, peaks, query):
    """One scan_records call over all 532 peaks with `query` (cached for the later tests)."""
    if query not in _PEAKS:
        engine.set_query(_rna(golden_dir, query))
        res = engine.scan_records([s for _, s in peaks], mod.default_params(cLength=20))
        _PEAKS[query] = (res, engine.last_totals[0])
    return _PEAKS[query]


# ---- 1. the reference's peaks, one call per lncRNA ---------------------------------------------------------------------------
@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_peaks_against_reference(mod, engine, golden_dir, peaks, query):
    res, tot = _peak_results(mod, engine, golden_dir, peaks, query)
    man = helpers.read_manifest(os.path.join(golden_dir, f"peaks_{query}.manifest.gz"))
    assert len(res) == NREC
    bad = []
    for r, x in zip(man, res):
        trips = x.triplexes()
        if (len(trips), helpers.triplex_digest(trips)) != (r["triplexes"], r["triplex_sha"]):
            bad.append(f"record {r['idx']} ({r['header']}): {len(trips)} triplexes, reference {r['triplexes']}")
        assert x.stats["units"] == NENC and x.stats["segments"] == 1, r["idx"]
        assert x.stats["t_total_s"] == 0 and sum(x.stats["kernel_launches"]) == 0
    assert not bad, bad
    assert tot["units"] == NREC * NENC and tot["segments"] == NREC
    assert tot["candidates"] == sum(x.stats["candidates"] for x in res)
    assert tot["t_total_s"] > 0 and sum(tot["kernel_launches"]) > 0


# ---- 2. three lncRNAs in one call ----------------------------------------------------------------------------------------------
def test_three_queries_in_one_call(mod, engine, golden_dir, peaks):
    p = mod.default_params(cLength=20)
    rnas = [_rna(golden_dir, q) for q in helpers.PEAK_QUERIES]
    dnas = [s for _, s in peaks]
    multi = engine.scan_records(dnas, p, rnas=rnas)
    assert len(multi) == 3 and len(engine.last_totals) == 3
    for q, name in enumerate(helpers.PEAK_QUERIES):
        single, _ = _peak_results(mod, engine, golden_dir, peaks, name)
        for r in range(NREC):
            assert _same(multi[q][r], single[r]), (name, r)
            assert [multi[q][r].stats[k] for k in SEVEN] == [single[r].stats[k] for k in SEVEN], (name, r)
        engine.set_query(rnas[q])
        for r in range(0, NREC, 16):
            alone = engine.scan(dnas[r], p)
            assert _same(multi[q][r], alone), (name, r)
            assert [multi[q][r].stats[k] for k in SEVEN] == [alone.stats[k] for k in SEVEN], (name, r)


# ---- 3. reference files inside a set -------------------------------------------------------------------------------------------
def test_reference_files_inside_a_set(mod, engine, golden_dir, peaks):
    p = mod.default_params(cLength=40)
    named = [synth.read_fasta(os.path.join(golden_dir, f)) for f in ("testDNA.fa", "planted40k.fa")]
    recs = [peaks[3], named[0], peaks[100], named[1], peaks[400]]
    engine.set_query(_rna(golden_dir, "H19"))
    res = engine.scan_records([s for _, s in recs], p)
    assert res[3].stats["segments"] == 9
    for k, gold in ((1, "demo_lg40"), (3, "planted40k")):
        hdr, dna = recs[k]
        _, chro, start = mod.parse_dna_header(hdr)
        tfo, c1, c2 = mod.tail_outputs(res[k], chro, start, len(dna), "H19", p)
        assert tfo == open(os.path.join(golden_dir, gold + ".TFOsorted"), "rb").read(), gold
        assert c1 == open(os.path.join(golden_dir, gold + ".TFOclass1"), "rb").read(), gold
        assert c2 == open(os.path.join(golden_dir, gold + ".TFOclass2"), "rb").read(), gold


# ---- 4-6. a mixed set against single scans, shards, resident --------------------------------------------------------------------
def _mixed_set(golden_dir):
    h19 = _rna(golden_dir, "H19")
    rnd = lambda n, s: synth.random_dna(n, s)
    recs = [rnd(20, 1), rnd(99, 2), rnd(150, 3), rnd(4899, 4), rnd(4900, 5), rnd(4901, 6), rnd(5000, 7), rnd(5001, 8),
            synth.planted_dna(9800, 9, h19, every=900), rnd(9801, 10), synth.planted_dna(12345, 11, h19, every=1100),
            synth.read_fasta(os.path.join(golden_dir, "planted40k.fa"))[1], b"N" * 3000, b"A" * 2500,
            synth.read_fasta(os.path.join(golden_dir, "messy.fa"))[1]]
    for k in range(15):
        n = 2000 + (k * 7919) % 1000
        recs.append(synth.planted_dna(n, 100 + k, h19, every=600) if k % 3 == 0 else rnd(n, 100 + k))
    return recs


_MIXED = {}


def _mixed_singles(mod, engine, golden_dir, p):
    if "single" not in _MIXED:
        engine.set_query(_rna(golden_dir, "H19"))
        _MIXED["single"] = [engine.scan(d, p) for d in _mixed_set(golden_dir)]
    return _MIXED["single"]


@pytest.mark.parametrize("opts", [{}, {"seg_batch": 1}, {"seg_batch": 3}, {"seg_batch": 7}, {"workers": 1}, {"workers": 16}],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_mixed_set_equals_single_scans(mod, engine, golden_dir, opts):
    p = mod.default_params(cLength=20)
    dnas = _mixed_set(golden_dir)
    singles = _mixed_singles(mod, engine, golden_dir, p)
    e = mod.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_query(_rna(golden_dir, "H19"))
    res = e.scan_records(dnas, p)
    tot = e.last_totals[0]
    e.close()
    assert sum(x.count for x in singles) > 0
    assert singles[13].stats["segments_skipped"] == 1          # the all-A record: same_seq()
    for r, (x, s) in enumerate(zip(res, singles)):
        assert _same(x, s), (opts, r, len(dnas[r]))
        assert [x.stats[k] for k in SEVEN] == [s.stats[k] for k in SEVEN], (opts, r, len(dnas[r]))
    assert tot["units"] == sum(s.stats["units"] for s in singles)
    if not opts:
        _MIXED["default"] = res


def test_mixed_set_short_records_against_oracle(mod, engine, golden_dir, oracle_build, tmp_path):
    """Records under 5 kb of the mixed set: the set's -TFOsorted equals the CPU oracle's (the reference's arithmetic)."""
    p = mod.default_params(cLength=20)
    dnas = _mixed_set(golden_dir)
    engine.set_query(_rna(golden_dir, "H19"))
    res = engine.scan_records(dnas, p)
    checked = 0
    for r, d in enumerate(dnas):
        if len(d) >= 5000 or r in (12, 13) or (r > 15 and r % 3):
            continue
        fa = tmp_path / f"r{r}.fa"
        fa.write_bytes(b">syn|chrT|1-%d\n" % len(d) + d + b"\n")
        exp = helpers.oracle_cli(oracle_build, "tfosorted", os.path.join(golden_dir, "H19.fa"), str(fa), "-lg", "20", "-threads", "8")
        assert mod.tfosorted(res[r], "chrT", 1, p) == exp, (r, len(d))
        checked += 1
    assert checked >= 8


def test_shards_merge_to_the_whole_call(mod, engine, golden_dir):
    p = mod.default_params(cLength=20)
    dnas = _mixed_set(golden_dir)
    engine.set_query(_rna(golden_dir, "H19"))
    whole = engine.scan_records(dnas, p)
    first = [0]
    for d in dnas:
        first.append(first[-1] + mod.segment_count(len(d), p))
    assert first[12] - first[11] == 9                         # planted40k: cut inside it and inside the 12 345-nt record
    cuts = [0, first[10] + 1, first[11] + 4, first[-1]]
    parts = [engine.scan_records(dnas, p, seg_first=cuts[i], seg_count=cuts[i + 1] - cuts[i]) for i in range(3)]
    for r in range(len(dnas)):
        merged = mod.merge_results([parts[i][r] for i in range(3)])
        assert _same(merged, whole[r]), r
    assert parts[0][-1].count == 0 and parts[0][-1].stats["segments"] == 0


def test_resident_set(mod, engine, golden_dir):
    p = mod.default_params(cLength=20)
    dnas = _mixed_set(golden_dir)
    engine.set_query(_rna(golden_dir, "H19"))
    host = _MIXED.get("default") or engine.scan_records(dnas, p)
    engine.load_dna(b"".join(dnas))
    res = engine.scan_records(None, p, rec_lens=[len(d) for d in dnas])
    for r in range(len(dnas)):
        assert _same(res[r], host[r]), r
        assert [res[r].stats[k] for k in SEVEN] == [host[r].stats[k] for k in SEVEN], r


# ---- 7. switches ---------------------------------------------------------------------------------------------------------------
_SWITCHES = {
    "band0": ({"band": 0}, {}), "band1": ({"band": 1}, {}), "band2": ({"band": 2}, {}),
    "hazard_whole_unit": ({"hazard_chunks": 0}, {}), "hazard_snapshots": ({"hazard_snapshots": 1}, {}),
    "scan_v1": ({}, {"FASIM_SCAN_V1": "1"}), "align_v1": ({}, {"FASIM_ALIGN_V1": "1"}), "striped_window": ({"striped_window": 1}, {}),
}


@pytest.mark.parametrize("switch", sorted(_SWITCHES))
def test_switches_on_peaks(mod, engine, golden_dir, peaks, monkeypatch, switch):
    base, _ = _peak_results(mod, engine, golden_dir, peaks, "H19")
    opts, env = _SWITCHES[switch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = mod.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_query(_rna(golden_dir, "H19"))
    res = e.scan_records([s for _, s in peaks], mod.default_params(cLength=20))
    e.close()
    assert sum(x.count for x in base) > 0
    for r in range(NREC):
        assert _same(res[r], base[r]), (switch, r)


# ---- 8. long query (> 16 tiles: the batch cut of the tile rule) -----------------------------------------------------------------
def test_long_query_records(mod, engine, golden_dir, peaks):
    p = mod.default_params(cLength=20)
    dnas = [synth.read_fasta(os.path.join(golden_dir, "longq_dna.fa"))[1], peaks[7][1], synth.random_dna(3000, 77), peaks[200][1]]
    engine.set_query(_rna(golden_dir, "longq49k"))
    res = engine.scan_records(dnas, p)
    for r, d in enumerate(dnas):
        alone = engine.scan(d, p)
        assert _same(res[r], alone), r
        assert [res[r].stats[k] for k in SEVEN] == [alone.stats[k] for k in SEVEN], r
    assert res[0].count > 0


# ---- 9. -F ---------------------------------------------------------------------------------------------------------------------
def test_classic_sim_records(mod, engine, golden_dir):
    p = mod.default_params(cLength=40, classicSim=1)
    hdr, demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))
    dnas = [demo, demo[:1200], demo[1200:2400], demo[-1200:]]
    engine.set_query(_rna(golden_dir, "H19"))
    res = engine.scan_records(dnas, p)
    for r, d in enumerate(dnas):
        alone = engine.scan(d, p)
        assert _same(res[r], alone), r
        assert [res[r].stats[k] for k in SEVEN] == [alone.stats[k] for k in SEVEN], r
    _, chro, start = mod.parse_dna_header(hdr)
    assert mod.tfosorted(res[0], chro, start, p) == open(os.path.join(golden_dir, "demoF_lg40.TFOsorted"), "rb").read()


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mod, golden_dir, peaks):
    p = mod.default_params(cLength=20)
    e = mod.Engine(0)
    e.set_query(_rna(golden_dir, "H19"))
    dnas = [s for _, s in peaks[:3]]
    with pytest.raises(mod.FasimError) as x:
        e.scan_records([], p)
    assert x.value.code == mod.E_ARG and "nrec" in str(x.value)
    with pytest.raises(mod.FasimError) as x:
        e.scan_records([dnas[0], b"", dnas[1]], p)
    assert x.value.code == mod.E_ARG and "record 1" in str(x.value)
    e.load_dna(b"".join(dnas))
    with pytest.raises(mod.FasimError) as x:
        e.scan_records(None, p, rec_lens=[len(dnas[0]), len(dnas[1]), len(dnas[2]) + 1])
    assert x.value.code == mod.E_ARG and "record 2" in str(x.value)
    with pytest.raises(mod.FasimError) as x:
        e.scan_records(dnas, p, rnas=[b"ACGT" * 10, b"A" * (mod.MAX_QUERY + 1)])
    assert x.value.code == mod.E_UNSUPPORTED and "query 1" in str(x.value)
    res = e.scan_records(dnas, p)
    e.set_query(_rna(golden_dir, "H19"))
    for r in range(3):
        assert _same(res[r], e.scan(dnas[r], p)), r
    e.close()


# ---- 11-12. the CLI ------------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, name, dna_file, rna_file, env_group, extra=()):
    exe = os.path.join(entry.PKG_DIR, "fasim")
    out = tmp_path / name
    out.mkdir()
    env = dict(os.environ)
    env.pop("FASIM_RECORD_GROUP", None)
    if env_group is not None:
        env["FASIM_RECORD_GROUP"] = str(env_group)
    r = subprocess.run([exe, "-f1", dna_file, "-f2", rna_file, "-O", f"{name}/", "--all-records", "--stats", *extra], cwd=tmp_path,
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
    files = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}
    return files, r.stderr.decode()


def test_cli_peaks_grouped_equals_per_record(golden_dir, tmp_path):
    (tmp_path / "peaks.fa").write_bytes(helpers.gunzip(os.path.join(golden_dir, "meg3_peaks.fa.gz")))
    (tmp_path / "H19.fa").write_bytes(open(os.path.join(golden_dir, "H19.fa"), "rb").read())
    grouped, err_g = _run_cli(tmp_path, "grouped", "peaks.fa", "H19.fa", None)
    single, err_s = _run_cli(tmp_path, "single", "peaks.fa", "H19.fa", 0)
    assert len(grouped) == NREC * 3 and grouped == single
    assert "[fasim] group 0:" in err_g and "[fasim] group" not in err_s
    rec_lines = lambda err: [l for l in err.splitlines() if l.startswith("[fasim] record")]
    assert rec_lines(err_g) == rec_lines(err_s) and len(rec_lines(err_g)) == NREC
    man = helpers.read_manifest(os.path.join(golden_dir, "peaks_H19.manifest.gz"))
    rna_name = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[0]
    for r in man:
        species, chro = r["header"].split("|")[:2]
        stem = f"{species}-{rna_name}-peaks.{chro}"
        assert helpers.file_digest(grouped[f"{stem}-TFOsorted"]) == (r["TFOsorted_lines"], r["TFOsorted_sha"]), r["idx"]
        for level in (1, 2):
            got = helpers.file_digest(grouped[f"{stem}-TFOclass{level}-15-50"])
            assert got == (r[f"TFOclass{level}_lines"], r[f"TFOclass{level}_sha"]), (r["idx"], level)


def test_cli_mixed_file_groups_flushes_and_devices(golden_dir, peaks, tmp_path):
    h19 = _rna(golden_dir, "H19")
    lines = []
    for k in range(30):
        lines.append(f">hg19|pk{k}|{1000 * k + 1}-{1000 * k + 3000}".encode())
        lines.append(peaks[k * 17][1])
        if k == 12:
            big = synth.planted_dna(1_200_000, 4242, h19, every=5000)
            lines += [b">syn|chrBig|1-1200000", big]
    (tmp_path / "mixed.fa").write_bytes(b"\n".join(lines) + b"\n")
    (tmp_path / "two.fa").write_bytes(open(os.path.join(golden_dir, "H19.fa"), "rb").read() +
                                      open(os.path.join(golden_dir, "MEG3.fa"), "rb").read())
    ref, _ = _run_cli(tmp_path, "ref", "mixed.fa", "two.fa", 0)
    assert len(ref) == 31 * 2 * 3
    got, err = _run_cli(tmp_path, "g64", "mixed.fa", "two.fa", 64)
    assert got == ref and err.count("[fasim] group") == 2
    got, err = _run_cli(tmp_path, "g64d", "mixed.fa", "two.fa", 64, ("--devices", "0,0,0"))
    assert got == ref
    assert any(len(v) > 0 and v.count(b"\n") > 1 for k, v in ref.items() if "chrBig" in k and k.endswith("TFOsorted"))
