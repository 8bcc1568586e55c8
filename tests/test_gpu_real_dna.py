"""The reference's only real input, 532 human ChIP peak records (tests/golden/meg3_peaks.fa.gz), through the HIP path with MEG3,
H19 and MALAT1 as queries, against the reference's outputs for every record (`make_golden.py peaks`).  GPU only."""
import os
import subprocess

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

NREC, NENC = 532, 48


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


def _rna(golden_dir, query):
    return synth.read_fasta(os.path.join(golden_dir, query + ".fa"))[1]


def _rna_name(golden_dir, query):
    """The lncRNA's FASTA header, which the reference puts into file names and bedGraph track names (MEG3-ENST00000451743)."""
    return synth.read_fasta(os.path.join(golden_dir, query + ".fa"))[0]


def _manifest(golden_dir, query):
    return helpers.read_manifest(os.path.join(golden_dir, f"peaks_{query}.manifest.gz"))


def _detail_scans(golden_dir, query):
    scans = helpers.split_sections(helpers.gunzip(os.path.join(golden_dir, f"peaks_{query}.detail.scan.gz")))
    return {i: helpers.parse_scan(s)[1] for (i, _), s in scans.items()}


def _where(r):
    return f"record {r['idx']} ({r['header']})"


# ---- a. the CLI over the whole file, one set of output files per record --------------------------------------------------------
@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_cli_every_peak_record(golden_dir, tmp_path, query):
    """`fasim --all-records` with default parameters writes the three files of every record under the reference's names (with the
    `.chr` suffix), each with the line count and SHA-256 of the file the reference CLI writes for that record alone."""
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "peaks.fa").write_bytes(helpers.gunzip(os.path.join(golden_dir, "meg3_peaks.fa.gz")))
    (tmp_path / f"{query}.fa").write_bytes(open(os.path.join(golden_dir, query + ".fa"), "rb").read())
    (tmp_path / "out").mkdir()
    subprocess.run([exe, "-f1", "peaks.fa", "-f2", f"{query}.fa", "-O", "out/", "--all-records"], cwd=tmp_path, check=True,
                   stdout=subprocess.DEVNULL)
    man = _manifest(golden_dir, query)
    stored = helpers.split_sections(helpers.gunzip(os.path.join(golden_dir, f"peaks_{query}.detail.files.gz")))
    rna_name = _rna_name(golden_dir, query)
    names = {}
    for r in man:
        species, chro = r["header"].split("|")[:2]
        stem = f"{species}-{rna_name}-peaks.{chro}"
        names[f"{stem}-TFOsorted"] = (r, "TFOsorted")
        for level in (1, 2):
            names[f"{stem}-TFOclass{level}-15-50"] = (r, f"TFOclass{level}")
    assert len(names) == NREC * 3
    assert sorted(os.listdir(tmp_path / "out")) == sorted(names)
    bad = []
    for name, (r, kind) in names.items():
        data = (tmp_path / "out" / name).read_bytes()
        if helpers.file_digest(data) != (r[kind + "_lines"], r[kind + "_sha"]):
            bad.append((r, kind, data))
    for r, kind, data in bad:
        if (r["idx"], kind) in stored:      # a record stored in full: show the difference
            assert data.decode() == stored[(r["idx"], kind)].decode(), f"{_where(r)} {kind}"
    assert not bad, [f"{_where(r)} {kind}" for r, kind, _ in bad]


# ---- b. the raw kernels, unit by unit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_unit_summaries_every_peak_record(mod, engine, golden_dir, peaks, query):
    """All 48 units of every record through pre_align_batch: stage-1 maximum, threshold, column-maximum hash and candidate count
    fold to the manifest's unit-summary digest of the reference's scan; the selected records are compared unit by unit."""
    engine.set_query(_rna(golden_dir, query))
    man = _manifest(golden_dir, query)
    detail = _detail_scans(golden_dir, query)
    bad = []
    chunk = 32
    for c0 in range(0, NREC, chunk):
        recs = peaks[c0:c0 + chunk]
        targets = [mod.encode_unit(seq, enc)[0] for _, seq in recs for enc in range(NENC)]
        cols, s1 = engine.pre_align_batch(targets)
        hashes = helpers.fnv1a_rows(cols)
        for k in range(len(recs)):
            r = man[c0 + k]
            units = []
            for enc in range(NENC):
                u = k * NENC + enc
                thr = int(s1[u] * 0.8)                      # Fasim-LongTarget.cpp:413
                units.append((enc, s1[u], thr, hashes[u], len(mod.pick_candidates(cols[u], thr))))
            if r["idx"] in detail:
                for got, ref in zip(units, detail[r["idx"]]):
                    exp = (ref["enc"], ref["stage1"], ref["thr"], ref["colhash"], ref["ncand"])
                    assert got == exp, f"{_where(r)} enc {ref['enc']}: (enc, stage1, thr, colhash, ncand) {got} != {exp}"
            if helpers.unit_summary_digest(units) != r["units"]:
                bad.append(_where(r))
    assert not bad, bad


@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_scan_selected_peak_records_triplex_by_triplex(mod, engine, golden_dir, peaks, query):
    """Every fastSIM triplex of the selected records (highest stage-1, most Q1 / Q2 units, most triplexes, shortest, longest), bit
    for bit (identity / stability as float bits), and the candidate count."""
    engine.set_query(_rna(golden_dir, query))
    p = mod.default_params(cLength=20)          # cLength == ntMin: LongTarget's tail filter == fastSIM's
    for i, units in _detail_scans(golden_dir, query).items():
        hdr, seq = peaks[i]
        res = engine.scan(seq, p)
        where = f"record {i} ({hdr})"
        assert res.stats["units"] == len(units) == NENC, where
        assert res.stats["candidates"] == sum(u["ncand"] for u in units), where
        assert res.triplexes() == helpers.expected_triplexes(units), where


# ---- c. every record through the scan, and the paths real DNA drives ------------------------------------------------------------
@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_scan_every_peak_record_and_path_coverage(mod, engine, golden_dir, peaks, query):
    """Every record scanned on its own: its fastSIM triplexes (count and digest) equal the reference's.  Summed over the records,
    the paths real DNA drives have run:

    - stage2_overflow_units >= the units whose reference stage-1 score is >= 251 (Q1), record by record.  Not equality: k_scan_post
      flags a unit (flag 2) when its own column maximum reaches 251; that maximum is the textbook one, which the reference's
      8-bit pass can only undershoot (its signed lazy-F exit, Q2, stops the F loop early and never raises a cell), so a unit may
      overflow on the HIP path while the reference's byte pass stayed below 251 and its stage-1 score with it.
    - hazard_units >= the units where Q2 changes the column maxima above the threshold (oracle fo_pre_align_noq2), record by
      record, as in test_q2_units_scan.
    - rev_exact > 0: window tries with forward scores in 148-250 took the exact reverse pass.
    - MALAT1: the systolic scan kernel ran (3 query tiles).
    - H19: exact_replays > 0.  In a scan (engine_stage3.cpp, stage3_range) it counts the candidates sent to the stripe-faithful
      replay: a tainted forward winner, a try scoring >= 148 without a usable exact reverse pass, or a k_finish status other than
      0.  The default path does replay, and H19 on these peaks sends 8 candidates there.  Those triggers are the HIP kernels' own
      flags, not something the reference's output shows, so MALAT1 (0 on these peaks) and MEG3 are only reported.
      (engine_stage3.cpp:560, which counts only k_finish status 2, belongs to the batch align API, not to the scan.)"""
    engine.set_query(_rna(golden_dir, query))
    man = _manifest(golden_dir, query)
    p = mod.default_params(cLength=20)
    keys = ("units", "candidates", "stage2_overflow_units", "hazard_units", "rev_exact", "exact_replays")
    tot = dict.fromkeys(keys, 0)
    tot["systolic_launches"] = 0
    bad = []
    for r, (hdr, seq) in zip(man, peaks):
        res = engine.scan(seq, p)
        st = res.stats
        for k in keys:
            tot[k] += st[k]
        tot["systolic_launches"] += st["kernel_launches"][0]
        trips = res.triplexes()
        if (len(trips), helpers.triplex_digest(trips)) != (r["triplexes"], r["triplex_sha"]):
            bad.append(f"{_where(r)}: {len(trips)} triplexes, reference {r['triplexes']}")
        assert st["units"] == NENC, _where(r)
        assert st["stage2_overflow_units"] >= r["q1"], _where(r)
        if r["q2"] is not None:
            assert st["hazard_units"] >= r["q2"], _where(r)
    q1, rev148 = sum(r["q1"] for r in man), sum(r["rev148"] for r in man)
    q2 = sum(r["q2"] for r in man) if query != "MEG3" else None
    print(f"\npeaks x {query}: HIP {tot}; reference Q1 {q1}, stage-1 148-250 {rev148}, Q2 {q2}, "
          f"triplexes {sum(r['triplexes'] for r in man)}")
    assert not bad, bad
    assert tot["units"] == NREC * NENC
    if query in ("H19", "MALAT1"):
        assert q1 > 0 and q2 > 0
        assert tot["stage2_overflow_units"] >= q1
        assert tot["hazard_units"] >= q2
        assert tot["rev_exact"] > 0
    if query == "H19":
        assert tot["exact_replays"] > 0
    if query == "MALAT1":
        assert tot["systolic_launches"] > 0


# ---- d. the switches agree on the 532 sequences joined into one 1.3 Mb record ----------------------------------------------------
_SWITCHES = {
    "band0": ({"band": 0}, {}),
    "band1": ({"band": 1}, {}),
    "band2": ({"band": 2}, {}),
    "hazard_whole_unit": ({"hazard_chunks": 0}, {}),
    "hazard_chunks_from_col0": ({"hazard_chunks": 1, "hazard_snapshots": 0}, {}),
    "hazard_chunks_snapshots": ({"hazard_chunks": 1, "hazard_snapshots": 1}, {}),
    "hazard_small_chunks": ({"hazard_chunks": 1, "hazard_chunk_cols": 64, "hazard_hot_weight": 16}, {}),
    "scan_v1": ({}, {"FASIM_SCAN_V1": "1"}),
    "align_v1": ({}, {"FASIM_ALIGN_V1": "1"}),
    "striped_window": ({"striped_window": 1}, {}),
}
_DEFAULT = {}


def _joined(peaks):
    return b"".join(s for _, s in peaks)


def _scan_joined(mod, golden_dir, peaks, query, p, opts=None):
    e = mod.Engine(0)
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    e.set_query(_rna(golden_dir, query))
    r = e.scan(_joined(peaks), p)
    e.close()
    return r


@pytest.mark.parametrize("switch", sorted(_SWITCHES))
@pytest.mark.parametrize("query", ["H19", "MALAT1"])
def test_switches_agree_on_joined_peaks(mod, golden_dir, peaks, monkeypatch, query, switch):
    """Band modes, the four organisations of the hazard re-run, the stripe-faithful scan / align kernels everywhere and the
    HBM-window striped kernel give the default's records and candidates on real DNA."""
    p = mod.default_params(cLength=20)
    if query not in _DEFAULT:
        d = _scan_joined(mod, golden_dir, peaks, query, p)
        _DEFAULT[query] = (d.recs, d.pool, d.stats["candidates"], d.count)
    opts, env = _SWITCHES[switch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = _scan_joined(mod, golden_dir, peaks, query, p, opts)
    assert _DEFAULT[query][3] > 0
    assert (r.recs, r.pool, r.stats["candidates"]) == _DEFAULT[query][:3], (query, switch, r.count, _DEFAULT[query][3])


@pytest.mark.parametrize("query", ["MEG3", "H19"])
def test_joined_peaks_files_and_sharding(mod, golden_dir, peaks, query):
    """All 532 sequences as one record (multi-segment scan, overlaps across record junctions, full-size batches of real DNA) with
    default parameters: the three files equal the reference CLI's (peaks_cat_<query>.manifest), also when the scan is cut into
    three segment shards and merged."""
    dna = _joined(peaks)
    exp = {}
    for line in open(os.path.join(golden_dir, f"peaks_cat_{query}.manifest")).read().splitlines():
        kind, n, sha = line.split("\t")
        exp[kind] = (int(n), sha)
    p = mod.default_params()
    e = mod.Engine(0)
    e.set_query(_rna(golden_dir, query))
    whole = e.scan(dna, p)
    nseg = mod.segment_count(len(dna), p)
    cuts = [0, nseg // 3, 2 * nseg // 3, nseg]
    parts = [e.scan(dna, p, cuts[i], cuts[i + 1] - cuts[i]) for i in range(3)]
    e.close()
    merged = mod.merge_results(parts)
    assert merged.recs == whole.recs and merged.pool == whole.pool
    import hashlib
    for res in (whole, merged):
        files = {"TFOsorted": mod.tfosorted(res, "chrP", 1, p)}
        for level in (1, 2):
            files[f"TFOclass{level}"] = mod.tfoclass(res, level, "chrP", 1, len(dna), _rna_name(golden_dir, query), p)
        for kind, data in files.items():
            assert (data.count(b"\n"), hashlib.sha256(data).hexdigest()) == exp[kind], kind
