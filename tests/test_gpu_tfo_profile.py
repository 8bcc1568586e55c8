"""The lncRNA's per-base profile on the GPU (fasim_scan_tfo_profile: the ROWS variant of k_scan, csrc/rowfold.hip) against the numpy
restatement of test_tfo_profile_cpu.py, which never calls the code under test: every unit of the demo, the drain columns at
segment ends, every row layout and tile count, the f16 switch and its integer re-run, independence of batches, workers, shards and
stage 3, per-record profiles of real peaks, refusals, and the CLI.  All array comparisons are exact.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_gpu_track import _chromosome_like
from test_tfo_profile_cpu import expected_profile, expected_profiles

pytestmark = pytest.mark.gpu

STATS = ("segments", "segments_skipped", "units", "candidates", "align_calls", "hazard_units", "stage2_overflow_units")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _seq(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _engine(mod, rna, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_query(rna)
    return e


def _profile(mod, rna, dnas, p=None, seg_first=0, seg_count=-1, **options):
    """profile-only call (no stage 3) on a fresh engine"""
    e = _engine(mod, rna, **options)
    none, prof = e.scan_tfo_profile(dnas, p, records=False, seg_first=seg_first, seg_count=seg_count)
    e.close()
    assert none is None
    return prof


def _same(got, want, what=""):
    """exact equality of (4, m) arrays, with the first differences in the message"""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), [(int(c), int(x), int(got[c, x]), int(want[c, x])) for c, x in bad[:6]])


def _random_rna(n, seed):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=n).tobytes())


def test_demo_equals_the_restatement(mod, golden_dir):
    """H19 x testDNA, defaults: all 48 units, the ones the reference cuts off at 250 and the hazard units included."""
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params()
    want, units = expected_profile(rna, [dna], p)
    print("largest row maximum per class:", want.max(axis=1).tolist())
    assert units == 48 and int(want.max()) > 250
    got = _profile(mod, rna, dna, p)
    assert (got.m, got.units, got.saturated_units) == (len(rna), 48, 0)
    arr = got.array()
    assert arr.dtype == np.uint16
    _same(arr, want)


def test_row_maxima_top_the_potential_tracks(mod, golden_dir):
    """Fact 1: max_i R[c][i] == max_x P[c][x] of the bin = 1 track of the same engine, on planted40k and on the chromosome-like
    30 kb record (a skipped segment, N runs, lower case)."""
    rna = _seq(golden_dir, "H19")
    for name, dna, p in (("planted40k", _seq(golden_dir, "planted40k"), mod.default_params()),
                         ("chromosome-like", _chromosome_like(), mod.default_params(rule=1, strand=0))):
        e = _engine(mod, rna)
        _, trk = e.scan_track(dna, p, bin=1, records=False)
        _, prof = e.scan_tfo_profile(dna, p, records=False)
        e.close()
        tops = trk.array().max(axis=1).tolist()
        print(name, "class maxima:", tops)
        assert max(tops) > 0
        assert prof.array().max(axis=1).tolist() == tops, name
        assert prof.units == trk.units


def test_hit_at_the_end_of_a_segment(mod):
    """The drain trap.  The last 40 bases of the record are, under rule 1 (encoding 0 writes A as T and G as G), a perfect match
    of query rows [a, a + 40), so H[a + 40][n] = H[a + 39][n - 1] - 4 in the drain column n exceeds everything row a + 40 really
    holds (its best is the gap from row a + 39, 16 below).  As 5 000 nt a full segment ends there, as 5 037 nt a short last
    segment does; the mirror image at the record start does the same to the reversed encodings (encoding 1 writes A as G and T
    as T, and reverses)."""
    a = 1500
    rows = bytes(np.random.default_rng(11).choice(np.frombuffer(b"GT", dtype=np.uint8), size=40).tobytes())
    rna = bytearray(_random_rna(2000, 12))
    rna[a:a + 40] = rows
    rna = bytes(rna)
    assert synth.RULE_OUT[0][0] == "T" and synth.RULE_OUT[0][2] == "G" and synth.RULE_OUT[1][0] == "G" and synth.RULE_OUT[1][1] == "T"
    at_end = rows.translate(bytes.maketrans(b"TG", b"AG"))                  # encoding 0 turns it into `rows`
    at_start = rows.translate(bytes.maketrans(b"GT", b"AT"))[::-1]           # encoding 1 turns it into `rows`, at the unit's end
    p = mod.default_params(rule=1, strand=0)
    for n in (5000, 5037):
        body = synth.random_dna(n - 40, 99)
        for what, dna in (("end", body + at_end), ("start", at_start + body)):
            assert len(dna) == n
            want, _ = expected_profile(rna, [dna], p)
            top = int(want[:, a + 39].max())
            assert top >= 200
            assert int(want[:, a + 40].max()) < top - 4          # top - 4 is what an unmasked drain column would leave there
            _same(_profile(mod, rna, dna, p).array(), want, f"{n} nt, hit at the {what}")


@pytest.mark.parametrize("m", [113, 128, 1000, 3072, 3073, 7000])
def test_row_layouts_and_tiles(mod, m):
    """Seeded queries of 113 ... 7 000 nt: RP 1 ... 24, one to three tiles, halves that own RP and RP - 1 rows; a 6 kb record under
    rule 1, with the f16 and the integer main pass."""
    rna = _random_rna(m, 1000 + m)
    dna = synth.random_dna(6000, 17)
    p = mod.default_params(rule=1, strand=0)
    want, units = expected_profile(rna, [dna], p)
    assert units == 2 * 4
    for f16 in (0, 1):
        got = _profile(mod, rna, dna, p, dp_f16=f16)
        assert got.units == units
        _same(got.array(), want, f"m {m} dp_f16 {f16}")


@pytest.mark.parametrize("case", helpers.row_layout_cases(), ids=helpers.row_layout_case_id)
def test_row_layouts_planted(mod, case):
    """The ROWS and ROWS + F16 builds of every RP = 1 ... 24, in both row layouts, on the planted record of the rows-per-lane sweep
    (helpers.row_layout_inputs): under rule 1 its units hold exact 32-row hits of encodings 0, 12 and 13 that run into a stripe
    boundary, so the row maxima are those of real hits (148 or more), not of random DNA."""
    k, layout, m = case
    rna, dna, _ = helpers.row_layout_inputs(m)
    p = mod.default_params(rule=1, strand=0)
    want, units = expected_profile(rna, [dna], p)
    assert units == 2 * 4
    print(f"RP {k} {layout} m {m}: largest row maximum per class {want.max(axis=1).tolist()}")
    assert int(want.max()) >= 148
    for f16 in (0, 1):
        got = _profile(mod, rna, dna, p, dp_f16=f16)
        assert got.units == units
        _same(got.array(), want, f"RP {k} {layout} m {m} dp_f16 {f16}")


def test_unit_beyond_the_exact_range_is_rerun(mod, golden_dir):
    """The input of test_gpu_dp_f16.test_unit_beyond_the_exact_range_is_rerun: the f16 pass hands the units that score above
    1 023 to the integer kernel, whose ROWS variant overwrites their void rows."""
    rna = _seq(golden_dir, "H19")
    enc = 26
    pre = {o: b for b, o in zip("ATGC", synth.RULE_OUT[enc])}
    window = rna[700:960].decode().upper().replace("U", "T")
    dna = bytearray(synth.random_dna(3000, 4242))
    dna[1200:1200 + len(window)] = "".join(pre[ch] for ch in window).encode()
    dna = bytes(dna)
    p = mod.default_params(cLength=20)
    want, _ = expected_profile(rna, [dna], p)
    assert int(want.max()) > 1023
    e = _engine(mod, rna, dp_f16=1)
    res, prof = e.scan_tfo_profile(dna, p)
    e.close()
    assert e.last_totals[0]["dp_f16_reruns"] > 0
    _same(prof.array(), want, "integer re-run")
    _same(_profile(mod, rna, dna, p, dp_f16=0).array(), want, "integer main pass")


def test_independent_of_batches_workers_shards_and_stage3(mod, golden_dir):
    """Seven segments (one skipped) of chromosome-like DNA and two short records, MEG3, rule 1."""
    rna = _seq(golden_dir, "MEG3")
    dnas = [_chromosome_like(), synth.random_dna(1800, 5), synth.random_dna(5200, 6)]
    p = mod.default_params(rule=1, strand=0)
    nseg = sum(mod.segment_count(len(d), p) for d in dnas)
    assert nseg == 7 + 1 + 2
    want, units = expected_profile(rna, dnas, p)
    base = _profile(mod, rna, dnas, p)
    assert base.units == units == 9 * 4
    _same(base.array(), want, "default")
    for seg_batch, workers in ((1, 1), (1, 10), (3, 1), (3, 10)):
        got = _profile(mod, rna, dnas, p, seg_batch=seg_batch, workers=workers)
        assert np.array_equal(got.array(), base.array()) and got.units == units, (seg_batch, workers)
    for cuts in ((0, 4, nseg), (0, 3, 6, nseg)):
        parts = [_profile(mod, rna, dnas, p, seg_first=a, seg_count=b - a) for a, b in zip(cuts, cuts[1:])]
        _same(parts[0].array(), expected_profile(rna, dnas, p, 0, cuts[1])[0], f"shard [0, {cuts[1]})")
        merged = mod.merge_tfo_profiles(parts)
        assert np.array_equal(merged.array(), base.array()) and merged.units == units, cuts
    # with stage 3: the same arrays, and the records and stats of scan_records
    e = _engine(mod, rna)
    plain = e.scan_records(dnas, p)
    totals = e.last_totals
    res, prof = e.scan_tfo_profile(dnas, p)
    e.close()
    assert np.array_equal(prof.array(), base.array()) and prof.units == units
    assert sum(r.count for r in plain) > 0
    for r in range(len(dnas)):
        assert (res[r].count, res[r].recs, res[r].pool) == (plain[r].count, plain[r].recs, plain[r].pool), r
        for k in STATS:
            assert res[r].stats[k] == plain[r].stats[k], (r, k)
    for k in STATS:
        assert e.last_totals[0][k] == totals[0][k], k


def test_real_peaks_per_record(mod, golden_dir):
    """The first 12 real MEG3 ChIP peaks x MEG3 and H19 in one call with per_record: each profile is that record's alone and the
    restatement's, and the whole-set profile is their element-wise maximum."""
    rnas = [_seq(golden_dir, "MEG3"), _seq(golden_dir, "H19")]
    peaks = [d for _, d in helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:12]]
    p = mod.default_params()
    e = _engine(mod, rnas[0])
    _, per = e.scan_tfo_profile(peaks, p, rnas=rnas, per_record=True, records=False)
    _, whole = e.scan_tfo_profile(peaks, p, rnas=rnas, records=False)
    for q, rna in enumerate(rnas):
        want, _ = expected_profiles(rna, peaks, p)
        for r, dna in enumerate(peaks):
            assert per[q][r].m == len(rna) and per[q][r].units == 48 * mod.segment_count(len(dna), p)
            _same(per[q][r].array(), want[r], f"query {q} record {r}")
        for r in (0, 7):
            _, alone = e.scan_tfo_profile([peaks[r]], p, rnas=[rna], records=False)
            assert np.array_equal(alone[0].array(), per[q][r].array()), (q, r)
        _same(whole[q].array(), np.maximum.reduce([x.array() for x in per[q]]), f"query {q} whole set")
        assert whole[q].units == sum(x.units for x in per[q])
    e.close()


def test_refusals_leave_the_engine_usable(mod, golden_dir, monkeypatch):
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    short = _seq(golden_dir, "h19_100")
    assert len(short) < 113
    e = _engine(mod, rna)
    for kw, code in ((dict(dnas=[dna], rnas=[_random_rna(112, 3)]), mod.E_UNSUPPORTED), (dict(dnas=[dna], rnas=[rna, short]), mod.E_UNSUPPORTED),
                     (dict(dnas=[dna], params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED), (dict(dnas=[]), mod.E_ARG)):
        with pytest.raises(mod.FasimError) as ei:
            e.scan_tfo_profile(**kw)
        assert ei.value.code == code, (kw.keys(), str(ei.value))
        print(ei.value)
    p = mod.default_params(cLength=40)
    gold = open(os.path.join(golden_dir, "demo_lg40.TFOsorted"), "rb").read()
    e.set_query(rna)
    assert mod.tfosorted(e.scan(dna, p), "chr11", 2158478, p) == gold
    e.close()
    monkeypatch.setenv("FASIM_SCAN_V1", "1")
    v1 = _engine(mod, rna)
    monkeypatch.delenv("FASIM_SCAN_V1")
    with pytest.raises(mod.FasimError) as ei:
        v1.scan_tfo_profile([dna])
    assert ei.value.code == mod.E_UNSUPPORTED
    assert mod.tfosorted(v1.scan(dna, p), "chr11", 2158478, p) == gold
    v1.close()


def test_cli_writes_the_profile_table(mod, golden_dir, tmp_path):
    exe = os.path.join(entry.PKG_DIR, "fasim")
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params(cLength=40)
    want = mod.tfo_profile_tsv(_profile(mod, rna, dna, p), rna, "H19")
    assert want.count(b"\n") == 1 + len(rna)
    three = {"hg19-H19-testDNA-TFOsorted": "demo_lg40.TFOsorted", "hg19-H19-testDNA-TFOclass1-15-40": "demo_lg40.TFOclass1",
             "hg19-H19-testDNA-TFOclass2-15-40": "demo_lg40.TFOclass2"}
    name = "hg19-H19-testDNA-TFOprofile"

    def run(out, *extra, status=0, f1="testDNA.fa"):
        (tmp_path / out).mkdir()
        r = subprocess.run([exe, "-f1", f1, "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra], cwd=tmp_path,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        assert r.returncode == status, r.stderr.decode()
        return sorted(os.listdir(tmp_path / out))

    assert run("plain") == sorted(three)
    for out, extra in (("full", []), ("two", ["--devices", "0,0"])):
        assert run(out, "--tfo-profile", *extra) == sorted(list(three) + [name])
        for got, gold in three.items():
            assert (tmp_path / out / got).read_bytes() == (tmp_path / "plain" / got).read_bytes(), got
            assert (tmp_path / out / got).read_bytes() == open(os.path.join(golden_dir, gold), "rb").read(), got
        assert (tmp_path / out / name).read_bytes() == want
    assert run("only", "--tfo-profile-only") == [name]
    assert (tmp_path / "only" / name).read_bytes() == want
    # --all-records on 20 real peaks: one whole-set table, the same from two device shards
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:20]
    (tmp_path / "peaks.fa").write_bytes(b"".join(b">" + h.encode() + b"\n" + d + b"\n" for h, d in peaks))
    table = "H19-peaks.tfoprofile.tsv"
    assert run("set1", "--tfo-profile-only", "--all-records", f1="peaks.fa") == [table]
    assert run("set2", "--tfo-profile-only", "--all-records", "--devices", "0,0", f1="peaks.fa") == [table]
    one = (tmp_path / "set1" / table).read_bytes()
    assert one == (tmp_path / "set2" / table).read_bytes()
    assert one == mod.tfo_profile_tsv(_profile(mod, rna, [d for _, d in peaks], p), rna, "H19")
    assert table in run("set3", "--tfo-profile", "--all-records", f1="peaks.fa")
    assert (tmp_path / "set3" / table).read_bytes() == one
    (tmp_path / "r.bed").write_text("chr11\t2158500\t2159000\n")
    for k, extra in enumerate((["-F"], ["--accumulate-records"], ["--track", "25"], ["--screen", "--all-records"],
                               ["--screen", "--regions", "r.bed"])):
        for flag in ("--tfo-profile", "--tfo-profile-only"):
            assert run(f"bad{k}{flag[-4:]}", flag, *extra, status=2) == []


def test_untidy_query(mod):
    """helpers.dirty_case(700): a T-to-U stretch, a lower-case stretch and scattered N R Y n u, x 10 kb whose plants cross those rows
    (rule 8: 6 units).  The row maxima of the untidy rows themselves are part of the profile: a U row pairs like A, a lower-case row
    like its capital, and an N / IUPAC row only carries what the diagonal brought (-4)."""
    rna, dna = helpers.dirty_case(700)
    p = mod.default_params(rule=8, strand=0)
    want, units = expected_profile(rna, [dna], p)
    rows = helpers.dirty_rows(rna)
    tops = {k: int(want[:, r].max()) for k, r in rows.items()}
    print("largest row maximum per class:", want.max(axis=1).tolist(), "; over the untidy rows:", tops)
    assert units == 6 and min(tops.values()) >= 100
    for f16 in (1, 0):
        got = _profile(mod, rna, dna, p, dp_f16=f16)
        assert (got.m, got.units, got.saturated_units) == (len(rna), 6, 0)
        _same(got.array(), want, f"dp_f16 {f16}")
