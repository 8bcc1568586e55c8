"""Sites above a fixed potential on the GPU (fasim_scan_records_sites, k_sites, `fasim --sites`): exact equality of the (n, 6) site
arrays with the numpy restatement (test_sites_cpu.py on test_track_cpu.py, which never calls the code under test) over thresholds
and gaps; batches, workers, the f16 switch, resident DNA, shards; record ends; several query tiles; refusals; the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_sites_cpu import expected_potential, raw_runs, sites_from
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

SEVEN = ("segments", "segments_skipped", "units", "candidates", "align_calls", "logical_cells", "cells_stage2")
EXE = os.path.join(entry.PKG_DIR, "fasim")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _seq(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _engine(mod, rna=None, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    if rna is not None:
        e.set_query(rna)
    return e


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    first = next((i for i in range(min(len(got), len(want))) if got[i].tolist() != want[i].tolist()), min(len(got), len(want)))
    raise AssertionError((what, got.shape, want.shape, first, got[max(0, first - 1):first + 3].tolist(), want[max(0, first - 1):first + 3].tolist()))


@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    """Case 1: the 30.5 kb construction x MEG3 under rule 1, both strands (7 segments, one of them all N, one unit per class), its
    restatement (computed once, never changed) and the thresholds."""
    rna, dna = _seq(golden_dir, "MEG3"), _chromosome_like()
    p = mod.default_params(rule=1, strand=0)
    P, per_enc = expected_potential(rna, dna, p)
    P.setflags(write=False)
    top = int(P.max())
    median = int(np.median(P[P > 0]))
    return dict(rna=rna, dna=dna, p=p, P=P, per_enc=per_enc, top=top, median=median, vs=(1, median, int(0.8 * top), top, top + 1))


def _crosses(runs, x):
    return any(a <= x - 1 and x < b for a, b in runs)


# ---- 1. restatement, thresholds and gaps -------------------------------------------------------------------------------------------
def test_the_case_is_not_vacuous(chrom):
    P, p, n = chrom["P"], chrom["p"], len(chrom["dna"])
    step = p.cutLength - p.overlapLength
    assert (step, p.cutLength) == (4900, 5000) and chrom["vs"][1] > 1 and chrom["vs"][2] > chrom["vs"][1]
    per_class = [raw_runs(P[c], chrom["median"]) for c in range(4)]
    print("median", chrom["median"], "top", chrom["top"], "raw runs per class at the median", [len(r) for r in per_class])
    assert max(len(r) for r in per_class) >= 500
    runs = [r for rs in per_class for r in rs]
    slice_edges = [a + k for a in range(0, n, step) for k in (2040, 4080) if a + k < n]
    assert any(_crosses(runs, x) for x in slice_edges)
    assert any(_crosses(runs, a) for a in range(step, n, step))
    assert any(_crosses(runs, a + 100) for a in range(step, n, step))
    assert len(sites_from(P, chrom["per_enc"], chrom["top"] + 1)) == 0 and len(sites_from(P, chrom["per_enc"], chrom["top"])) >= 1


@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("records", [False, True])
def test_thresholds_and_gaps_equal_the_restatement(mod, chrom, gap, records):
    e = _engine(mod, chrom["rna"])
    plain = e.scan_records([chrom["dna"]], chrom["p"]) if records else None
    for v in chrom["vs"]:
        res, sites = e.scan_sites(chrom["dna"], chrom["p"], min_value=v, max_gap=gap, records=records)
        want = sites_from(chrom["P"], chrom["per_enc"], v, gap)
        s = sites[0]
        _same(s.array(), want, f"V {v} G {gap}")
        assert s.array().dtype == np.int64 and (s.units, s.saturated_units, s.min_value, s.max_gap, len(s)) == (24, 0, v, gap, len(want))
        assert s.raw_runs >= len(raw_runs(chrom["P"][0], v)) * (v <= chrom["top"])
        if records:
            x, y = res[0], plain[0]
            assert (x.count, x.recs, x.pool) == (y.count, y.recs, y.pool) and [x.stats[k] for k in SEVEN] == [y.stats[k] for k in SEVEN]
        else:
            assert res is None
    e.close()


# ---- 2. default parameters, real DNA -----------------------------------------------------------------------------------------------
def test_first_24_peaks_equal_the_restatement_and_the_peaks(mod, golden_dir):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dnas = [s for _, s in helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:24]]
    e = _engine(mod, rna)
    _, _, pk = e.scan_records_track(dnas, p, bin=0, records=False)
    got = {g: e.scan_sites(dnas, p, min_value=60, max_gap=g, records=False)[1] for g in (0, 5)}
    e.close()
    assert pk.shape == (24, 4, 3)
    nsites = 0
    for r, dna in enumerate(dnas):
        P, per_enc = expected_potential(rna, dna, p)
        assert len(per_enc) == 48
        for g in (0, 5):
            s = got[g][r]
            _same(s.array(), sites_from(P, per_enc, 60, g), f"record {r} G {g}")
            assert s.units == 48
            a = s.array()
            nsites += len(a)
            for c in range(4):
                mine = a[a[:, 0] == c]
                if pk[r, c, 0] < 60:
                    assert len(mine) == 0, (r, c, g)
                    continue
                best = mine[np.argmax(mine[:, 3])]                  # (argmax: the first on ties)
                assert best[[3, 4, 5]].tolist() == pk[r, c].tolist(), (r, c, g, best.tolist(), pk[r, c].tolist())
    assert nsites > 96


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(seg_batch=1, workers=1), dict(seg_batch=1, workers=16), dict(seg_batch=3, workers=1),
                                     dict(seg_batch=3, workers=16), dict(dp_f16=0), dict(dp_f16=1)])
def test_batches_workers_and_the_f16_switch(mod, chrom, options):
    want = sites_from(chrom["P"], chrom["per_enc"], chrom["median"], 0)
    e = _engine(mod, chrom["rna"], **options)
    _, sites = e.scan_sites([chrom["dna"]], chrom["p"], min_value=chrom["median"], records=False)
    e.close()
    _same(sites[0].array(), want, str(options))


def test_resident_dna_and_records(mod, chrom):
    want = sites_from(chrom["P"], chrom["per_enc"], chrom["median"], 0)
    e = _engine(mod, chrom["rna"])
    plain = e.scan_records([chrom["dna"]], chrom["p"])[0]
    res_s, streamed = e.scan_sites(chrom["dna"], chrom["p"], min_value=chrom["median"])
    e.load_dna(chrom["dna"])
    res_r, resident = e.scan_sites(None, chrom["p"], min_value=chrom["median"])
    e.close()
    _same(streamed[0].array(), want, "streamed")
    _same(resident[0].array(), want, "resident")
    assert resident[0].raw_runs == streamed[0].raw_runs
    for x in (res_s[0], res_r[0]):
        assert (x.count, x.recs, x.pool) == (plain.count, plain.recs, plain.pool)
        assert [x.stats[k] for k in SEVEN] == [plain.stats[k] for k in SEVEN]


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------
def test_shards_merge_to_the_whole(mod, chrom):
    rna, dna, p, v = chrom["rna"], chrom["dna"], chrom["p"], chrom["median"]
    e = _engine(mod, rna)
    parts = []
    for first, count in ((0, 3), (3, -1)):
        _, s = e.scan_sites(dna, p, min_value=v, max_gap=5, records=False, seg_first=first, seg_count=count)
        Pk, pk = expected_potential(rna, dna, p, first, count)
        _same(s[0].array(), sites_from(Pk, pk, v, 5), f"shard from {first}")
        parts.append(s[0])
    _, whole = e.scan_sites(dna, p, min_value=v, max_gap=5, records=False)
    e.close()
    merged = mod.merge_sites(parts)
    _same(merged.array(), sites_from(chrom["P"], chrom["per_enc"], v, 5), "merged")
    assert (parts[0].units, parts[1].units, merged.units) == (8, 16, 24)
    assert merged.raw_runs == parts[0].raw_runs + parts[1].raw_runs == whole[0].raw_runs


# ---- 5. record ends ------------------------------------------------------------------------------------------------------------------
def test_sites_at_the_ends_of_the_record(mod):
    """A 40-nt perfect match planted on the last bases of a full segment (5 000 nt), of a short last segment (5 037 nt) and,
    mirrored for the reversed encoding, on the first bases of the record (the construction of test_gpu_tfo_profile.py)."""
    a = 1500
    rows = bytes(np.random.default_rng(11).choice(np.frombuffer(b"GT", dtype=np.uint8), size=40).tobytes())
    rna = bytearray(np.random.default_rng(12).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=2000).tobytes())
    rna[a:a + 40] = rows
    rna = bytes(rna)
    at_end = rows.translate(bytes.maketrans(b"TG", b"AG"))
    at_start = rows.translate(bytes.maketrans(b"GT", b"AT"))[::-1]
    p = mod.default_params(rule=1, strand=0)
    e = _engine(mod, rna)
    for n in (5000, 5037):
        body = synth.random_dna(n - 40, 99)
        for what, dna in (("end", body + at_end), ("start", at_start + body)):
            P, per_enc = expected_potential(rna, dna, p)
            v = int(0.8 * P.max())
            assert P.max() >= 200
            want = sites_from(P, per_enc, v, 0)
            _, s = e.scan_sites(dna, p, min_value=v, records=False)
            _same(s[0].array(), want, f"{n} nt, hit at the {what}")
            got = s[0].array()
            if what == "end":
                assert (got[:, 2] == len(dna)).any()
            else:
                assert (got[:, 1] == 0).any()
    e.close()


# ---- 6. several query tiles ----------------------------------------------------------------------------------------------------------
def test_three_query_tiles(mod):
    rna = bytes(np.random.default_rng(8007).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=7000).tobytes())
    dna = synth.planted_dna(6000, 17, rna)
    p = mod.default_params(rule=1, strand=0)
    P, per_enc = expected_potential(rna, dna, p)
    v = int(0.8 * P.max())
    want = sites_from(P, per_enc, v, 0)
    assert len(want) >= 1
    for f16 in (0, 1):
        e = _engine(mod, rna, dp_f16=f16)
        _, s = e.scan_sites(dna, p, min_value=v, records=False)
        e.close()
        _same(s[0].array(), want, f"dp_f16 {f16}")
        assert s[0].units == 8


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mod, golden_dir, chrom, monkeypatch):
    rna, dna, p = chrom["rna"], chrom["dna"], chrom["p"]
    short = _seq(golden_dir, "h19_100")
    assert len(short) < 113
    e = _engine(mod, rna)
    cases = [(dict(min_value=0), mod.E_ARG), (dict(min_value=-1), mod.E_ARG), (dict(min_value=16384), mod.E_ARG),
             (dict(min_value=60, max_gap=-1), mod.E_ARG), (dict(min_value=60, rnas=[short]), mod.E_UNSUPPORTED),
             (dict(min_value=60, rnas=[rna, short]), mod.E_UNSUPPORTED),
             (dict(min_value=60, params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED)]
    for kw, code in cases:
        kw = dict(kw)
        kw.setdefault("params", p)
        with pytest.raises(mod.FasimError) as ei:
            e.scan_sites(dna, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
        print(ei.value)
    L, C = mod.lib(), __import__("ctypes")
    offs, lens = (C.c_int64 * 1)(0), (C.c_int64 * 1)(len(dna))
    rc = L.fasim_scan_records_sites(e._h, None, None, 0, dna, offs, lens, 1, 0, -1, C.byref(p), 60, 0, None, None, None)
    assert rc == mod.E_ARG
    e.set_query(short)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_sites(dna, p, min_value=60)
    assert ei.value.code == mod.E_UNSUPPORTED
    e.set_query(rna)
    _, s = e.scan_sites(dna, p, min_value=chrom["median"], records=False)
    e.close()
    _same(s[0].array(), sites_from(chrom["P"], chrom["per_enc"], chrom["median"], 0), "after the refusals")
    # FASIM_SCAN_V1=1 is read when the engine is created
    monkeypatch.setenv("FASIM_SCAN_V1", "1")
    e1 = _engine(mod, rna)
    monkeypatch.delenv("FASIM_SCAN_V1")
    with pytest.raises(mod.FasimError) as ei:
        e1.scan_sites(dna, p, min_value=60)
    e1.close()
    assert ei.value.code == mod.E_UNSUPPORTED


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------------
def _run(wd, *args, env=None, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_plain_run(mod, golden_dir, tmp_path):
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params(cLength=40)
    e = _engine(mod, rna)
    want = {g: mod.sites_bed(e.scan_sites(dna, p, min_value=100, max_gap=g, records=False)[1][0], "chr11", 2158478, "H19") for g in (0, 7)}
    e.close()
    assert want[0].startswith(b"# fasim sites lncRNA=H19 min_value=100 max_gap=0\nchr11\t") and want[0].count(b"\n") > 4
    assert all(len(line.split(b"\t")) == 8 for line in want[0].splitlines()[1:]) and want[7] != want[0]
    three = {"hg19-H19-testDNA-TFOsorted": "demo_lg40.TFOsorted", "hg19-H19-testDNA-TFOclass1-15-40": "demo_lg40.TFOclass1",
             "hg19-H19-testDNA-TFOclass2-15-40": "demo_lg40.TFOclass2"}
    gold = {n: open(os.path.join(golden_dir, f), "rb").read() for n, f in three.items()}
    name = "hg19-H19-testDNA-TFOsites-100"

    def run(out, *extra, status=0):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra, status=status)
        return _files(tmp_path / out)

    assert run("without") == gold
    assert run("full", "--sites", "100") == dict(gold, **{name: want[0]})
    assert run("two", "--sites", "100", "--devices", "0,0") == dict(gold, **{name: want[0]})
    assert run("only", "--sites", "100", "--sites-only") == {name: want[0]}
    assert run("gap", "--sites", "100", "--sites-gap", "7", "--sites-only") == {name: want[7]}
    (tmp_path / "r.bed").write_text("chr11\t2158500\t2159000\n")
    refused = (["--sites", "0"], ["--sites", "16384"], ["--sites", "-4"], ["--sites", "100", "--sites-gap", "-1"], ["--sites-gap", "3"],
               ["--sites-only"], ["--sites", "100", "-F"], ["--sites", "100", "--accumulate-records"], ["--sites", "100", "--track", "25"],
               ["--sites", "100", "--all-records", "--screen"], ["--sites", "100", "--tfo-profile"],
               ["--sites", "100", "--regions", "r.bed", "--screen-only"])
    for k, extra in enumerate(refused):
        assert run(f"refused{k}", *extra, status=2) == {}, extra


def test_cli_record_sets(mod, golden_dir, tmp_path):
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:24]
    (tmp_path / "MEG3.fa").write_bytes(open(os.path.join(golden_dir, "MEG3.fa"), "rb").read())
    lnc = synth.read_fasta(str(tmp_path / "MEG3.fa"))[0]
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    # --all-records: the 24 records, each with its own chromosome and start
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    e = _engine(mod, rna)
    _, sites = e.scan_sites([s for _, s in peaks], p, min_value=60, records=False)
    want = b"# fasim sites lncRNA=%s min_value=60 max_gap=0\n" % lnc.encode()
    for (h, s), st in zip(peaks, sites):
        name, chro, span = h.split("|")
        want += mod.sites_bed(st, chro, int(span.split("-")[0]), lnc, record_name=name, header=False)
    assert want.count(b"\n") > 24 and all(len(line.split(b"\t")) == 9 for line in want.splitlines()[1:])

    def run(out, f1, *extra, env=None):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", "MEG3.fa", "-O", out + "/", *extra, env=env)
        return _files(tmp_path / out)

    fname = f"{lnc}-recs.sites-60.bed"
    assert run("all", "recs.fa", "--all-records", "--sites", "60", "--sites-only") == {fname: want}
    assert run("all0", "recs.fa", "--all-records", "--sites", "60", "--sites-only", env={"FASIM_RECORD_GROUP": "0"}) == {fname: want}
    assert run("all2", "recs.fa", "--all-records", "--sites", "60", "--sites-only", "--devices", "0,0") == {fname: want}
    # --regions: overlapping, nested, repeated and unordered intervals of two chromosomes
    g = {"chrA": b"".join(s for _, s in peaks[:4]), "chrB": b"".join(s for _, s in peaks[4:6])}
    assert len(g["chrA"]) > 9000 and len(g["chrB"]) > 4000
    la, lb = len(g["chrA"]), len(g["chrB"])
    bed = ["chrB\t0\t4000\tchrB_head", "chrA\t1000\t5900\tlen4900", "chrA\t3000\t9000", "chrA\t3500\t4200\tinner",
           f"chrA\t{la - 3000}\t{la}\tchrA_tail", "chrA\t1000\t5900\tlen4900", f"chrB\t{lb - 1}\t{lb}"]
    (tmp_path / "g.bed").write_text("".join(x + "\n" for x in bed))
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + g["chrA"] + b"\n>chrB some description\n" + g["chrB"] + b"\n")
    regs = mod.read_bed(tmp_path / "g.bed")
    _, sites = e.scan_sites([g[r.chrom][r.start:r.end] for r in regs], p, min_value=60, max_gap=5, records=False)
    e.close()
    want = b"# fasim sites lncRNA=%s min_value=60 max_gap=5\n" % lnc.encode()
    for r, st in zip(regs, sites):
        want += mod.sites_bed(st, r.chrom, r.start + 1, lnc, record_name=r.name, header=False)
    assert want.count(b"\n") > 7
    fname = f"{lnc}-genome.sites-60.bed"
    args = ("genome.fa", "--regions", "g.bed", "--sites", "60", "--sites-gap", "5")
    assert run("reg", *args, "--sites-only") == {fname: want}
    assert run("reg0", *args, "--sites-only", env={"FASIM_RECORD_GROUP": "0"}) == {fname: want}
    assert run("reg2", *args, "--sites-only", "--devices", "0,0") == {fname: want}
    plain = run("plain", "genome.fa", "--regions", "g.bed")
    assert run("both", *args) == dict(plain, **{fname: want})


# ---- an untidy query ----------------------------------------------------------------------------------------------------------------
def test_untidy_query(mod):
    """helpers.dirty_case(700) (U, lower case, N R Y n u in the query) under rule 8, whose units hold the plants across those rows:
    sites at the top, at 0.8 of it and at the median against the restatement (U read as A, every other letter -4)."""
    rna, dna = helpers.dirty_case(700)
    p = mod.default_params(rule=8, strand=0)
    P, per_enc = expected_potential(rna, dna, p)
    top, median = int(P.max()), int(np.median(P[P > 0]))
    assert top >= 150
    e = _engine(mod, rna)
    for v in (top, int(0.8 * top), median):
        want = sites_from(P, per_enc, v)
        _, sites = e.scan_sites(dna, p, min_value=v, records=False)
        _same(sites[0].array(), want, f"V {v}")
        assert (sites[0].units, sites[0].saturated_units, len(sites[0])) == (6, 0, len(want)) and len(want) >= 1
    e.close()
