"""Potential tracks on the GPU (fasim_scan_track, csrc/track.hip): the arrays against the numpy restatement of
test_track_cpu.py (which never calls the code under test) and against the oracle's restatement of the reference on real DNA;
records unchanged; batches, workers, shards, bins, query tiles, the f16 switch; refusals; the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import bin_reduce, colmax_units, enabled_encodings, enc_class, encode_unit, expected_tracks

pytestmark = pytest.mark.gpu


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


def _track(mod, rna, dna, p=None, records=False, bin=1, seg_first=0, seg_count=-1, **options):
    e = _engine(mod, rna, **options)
    res, t = e.scan_track(dna, p, bin=bin, records=records, seg_first=seg_first, seg_count=seg_count)
    e.close()
    return (res, t) if records else t


def _same(got, want, what=""):
    """exact equality of (4, n) arrays, with the first differences in the message"""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), [(int(c), int(x), int(got[c, x]), int(want[c, x])) for c, x in bad[:6]])


def test_demo_equals_the_restatement(mod, golden_dir):
    """Demo, default parameters, bin = 1: all 48 units, the ones the reference cuts off at 250 and the hazard units included."""
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params()
    want, top = expected_tracks(rna, dna, p)
    print("largest column maximum per class:", top)
    assert max(top) > 250
    t = _track(mod, rna, dna, p)
    assert (t.bin, t.nbins, t.units, t.saturated_units) == (1, len(dna), 48, 0)
    _same(t.array(), want)


def test_real_peaks_equal_the_reference_maxima(mod, golden_dir, oracle_build):
    """The first 40 real MEG3 ChIP peak records x MEG3: per class the maximum of the oracle's (= the reference's) column maxima
    of the class's units.  They are the textbook ones while they stay below 148, so a (record, class) pair one of whose units
    reaches 148 is left out: 5 of the 160 pairs, 3.07 % of the values, on the oracle's side alone; more than 5 % fails."""
    orc = helpers.Oracle(oracle_build)
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:40]
    e = _engine(mod, rna)
    total = left_out = pairs_out = 0
    for k, (_, dna) in enumerate(peaks):
        want, top = expected_tracks(rna, dna, p, colmax=lambda q, ts: [orc.pre_align(q, t) for t in ts])
        _, t = e.scan_track(dna, p, records=False)
        got = t.array()
        for c in range(4):
            total += len(dna)
            if top[c] >= 148:
                left_out += len(dna)
                pairs_out += 1
                continue
            _same(got[c:c + 1], want[c:c + 1], f"record {k} class {c}")
    e.close()
    print(f"{pairs_out} of {4 * len(peaks)} (record, class) pairs left out = {100.0 * left_out / total:.2f} % of the values")
    assert left_out <= 0.05 * total


@pytest.mark.parametrize("dna_file", ["testDNA", "planted40k"])
def test_records_are_those_of_scan_queries(mod, golden_dir, dna_file):
    """out_results of scan_track is byte for byte what scan_queries returns, and the track of the same call is the track-only
    call's."""
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, dna_file)
    p = mod.default_params(cLength=40)
    e = _engine(mod, rna)
    plain = e.scan_queries([rna], dna, p)[0]
    res, trk = e.scan_track(dna, p, rnas=[rna], bin=25)
    none, only = e.scan_track(dna, p, rnas=[rna], bin=25, records=False)
    e.close()
    assert none is None and plain.count > 0
    assert (res[0].count, res[0].recs, res[0].pool) == (plain.count, plain.recs, plain.pool)
    for k in ("segments", "segments_skipped", "units", "candidates", "align_calls", "hazard_units", "stage2_overflow_units"):
        assert res[0].stats[k] == plain.stats[k], k
    assert trk[0].nbins == (len(dna) + 24) // 25 and int(trk[0].array().max()) > 0
    assert np.array_equal(trk[0].array(), only[0].array())
    assert trk[0].units == only[0].units == plain.stats["units"]


def _chromosome_like():
    """About 30 kb of chromosome-like DNA (soft-masked repeats in lower case, which count as N) with a short N run and one whole
    segment of N: segment 2 = [9 800, 14 800) is skipped by same_seq."""
    dna = bytearray(synth.genome_like(30500, 77, every=1500, telomere=0))
    dna[9800:14800] = b"N" * 5000
    dna[20000:20037] = b"N" * 37
    return bytes(dna)


def test_segments_batches_bins_and_shards(mod, golden_dir):
    """Seven segments (one skipped), MEG3, rule 1, both strands: four units per segment, one per class."""
    rna, dna = _seq(golden_dir, "MEG3"), _chromosome_like()
    p = mod.default_params(rule=1, strand=0)
    assert sorted(enc_class(e) for e in enabled_encodings(p)) == [0, 1, 2, 3]
    assert any(c in dna for c in b"acgt") and mod.segment_count(len(dna), p) == 7
    want, top = expected_tracks(rna, dna, p)
    print("largest column maximum per class:", top)
    base = _track(mod, rna, dna, p)
    assert (base.units, base.nbins) == (6 * 4, len(dna))
    _same(base.array(), want, "bin 1")
    assert not want[:, 9900:14700].any()         # only the neighbours' overlaps cover the N segment
    for width in (25, 4900):
        _same(_track(mod, rna, dna, p, bin=width).array(), bin_reduce(want, width), f"bin {width}")
    # overlaps across batch borders, any number of workers
    for seg_batch, workers in ((1, 1), (1, 16), (3, 1), (3, 16)):
        for width in (1, 25):
            got = _track(mod, rna, dna, p, bin=width, seg_batch=seg_batch, workers=workers)
            _same(got.array(), bin_reduce(want, width), f"seg_batch {seg_batch} workers {workers} bin {width}")
    # shards: the arrays span the whole record and merge by maximum
    for width in (1, 25):
        a = _track(mod, rna, dna, p, bin=width, seg_first=0, seg_count=3)
        b = _track(mod, rna, dna, p, bin=width, seg_first=3, seg_count=-1)
        assert a.nbins == b.nbins == (len(dna) + width - 1) // width
        _same(a.array(), bin_reduce(expected_tracks(rna, dna, p, 0, 3)[0], width), f"shard [0, 3) bin {width}")
        merged = mod.merge_tracks([a, b])
        _same(merged.array(), bin_reduce(want, width), f"merged shards bin {width}")
        assert merged.units == 24
    # the resident record gives what the streamed host buffer gives, with records too
    e = _engine(mod, rna)
    e.load_dna(dna)
    res, resident = e.scan_track(None, p, bin=25)
    res2, streamed = e.scan_track(dna, p, bin=25)
    e.close()
    _same(resident.array(), bin_reduce(want, 25), "resident")
    assert np.array_equal(resident.array(), streamed.array()) and (res.recs, res.pool) == (res2.recs, res2.pool)


def test_query_tiles_and_the_f16_switch(mod, golden_dir, oracle_build):
    """A 3-tile query (MALAT1), dp_f16 on and off, and a unit that the f16 pass hands to the integer kernel (scores above 1 023)."""
    p4 = mod.default_params(rule=1, strand=0)
    rna, dna = _seq(golden_dir, "MALAT1"), _seq(golden_dir, "malat1_dna")
    want, top = expected_tracks(rna, dna, p4)
    print("MALAT1: largest column maximum per class:", top)
    t1, t0 = _track(mod, rna, dna, p4, dp_f16=1), _track(mod, rna, dna, p4, dp_f16=0)
    _same(t1.array(), want, "MALAT1 dp_f16 1")
    _same(t0.array(), want, "MALAT1 dp_f16 0")
    h19, demo = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    assert np.array_equal(_track(mod, h19, demo, dp_f16=1).array(), _track(mod, h19, demo, dp_f16=0).array())
    # the pre-image of 260 nt of H19 under encoding 26 in 3 kb of random DNA (as in test_gpu_dp_f16.py)
    enc = 26
    pre = {o: b for b, o in zip("ATGC", synth.RULE_OUT[enc])}
    window = h19[700:960].decode().upper().replace("U", "T")
    dna = bytearray(synth.random_dna(3000, 4242))
    dna[1200:1200 + len(window)] = "".join(pre[ch] for ch in window).encode()
    dna = bytes(dna)
    p = mod.default_params()
    want, top = expected_tracks(h19, dna, p)
    print("pre-image record: largest column maximum per class:", top)
    assert top[enc_class(enc)] > 1023
    e = _engine(mod, h19, dp_f16=1)
    res, t = e.scan_track(dna, p)
    e.close()
    assert res.stats["dp_f16_reruns"] > 0
    _same(t.array(), want, "integer re-run")
    assert int(t.array().max()) > 1023


def test_refusals_leave_the_engine_usable(mod, golden_dir):
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    short = _seq(golden_dir, "h19_100")
    assert len(short) < 113
    e = _engine(mod, rna)
    for kw, code in ((dict(rnas=[short]), mod.E_UNSUPPORTED), (dict(rnas=[rna, short]), mod.E_UNSUPPORTED), (dict(bin=0), mod.E_ARG),
                     (dict(bin=-3), mod.E_ARG), (dict(params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED)):
        with pytest.raises(mod.FasimError) as ei:
            e.scan_track(dna, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
        print(ei.value)
    p = mod.default_params(cLength=40)
    gold = open(os.path.join(golden_dir, "demo_lg40.TFOsorted"), "rb").read()
    assert mod.tfosorted(e.scan(dna, p), "chr11", 2158478, p) == gold
    e.set_query(short)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_track(dna)
    assert ei.value.code == mod.E_UNSUPPORTED
    e.set_query(rna)
    assert mod.tfosorted(e.scan(dna, p), "chr11", 2158478, p) == gold
    e.close()


def test_cli_writes_the_track_file(mod, golden_dir, tmp_path):
    exe = os.path.join(entry.PKG_DIR, "fasim")
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params(cLength=40)
    want = mod.track_bedgraph(_track(mod, rna, dna, p, bin=25), "chr11", 2158478, len(dna), "H19")
    assert want.count(b"\n") > 4 + 40
    three = {"hg19-H19-testDNA-TFOsorted": "demo_lg40.TFOsorted", "hg19-H19-testDNA-TFOclass1-15-40": "demo_lg40.TFOclass1",
             "hg19-H19-testDNA-TFOclass2-15-40": "demo_lg40.TFOclass2"}
    name = "hg19-H19-testDNA-TFOpotential-25"

    def run(out, *extra, status=0):
        (tmp_path / out).mkdir()
        r = subprocess.run([exe, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra], cwd=tmp_path,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        assert r.returncode == status, r.stderr.decode()
        return sorted(os.listdir(tmp_path / out))

    for out, extra in (("full", []), ("two", ["--devices", "0,0"])):
        assert run(out, "--track", "25", *extra) == sorted(list(three) + [name])
        for got, gold in three.items():
            assert (tmp_path / out / got).read_bytes() == open(os.path.join(golden_dir, gold), "rb").read(), got
        assert (tmp_path / out / name).read_bytes() == want
    assert run("only", "--track", "25", "--track-only") == [name]
    assert (tmp_path / "only" / name).read_bytes() == want
    assert run("min", "--track", "25", "--track-only", "--track-min", "60") == [name]
    t = _track(mod, rna, dna, p, bin=25)
    assert (tmp_path / "min" / name).read_bytes() == mod.track_bedgraph(t, "chr11", 2158478, len(dna), "H19", min_value=60)
    (tmp_path / "r.bed").write_text("chr11\t2158500\t2159000\n")
    assert run("bed", "--track", "25", "--regions", "r.bed", status=2) == []
    assert run("acc", "--track", "25", "--accumulate-records", status=2) == []
    assert run("sim", "--track", "25", "-F", status=2) == []
    assert run("alone", "--track-only", status=2) == []


def test_untidy_query(mod):
    """A query with a T-to-U stretch, a lower-case stretch and scattered N R Y n u (helpers.dirty_case(700)) x 10 kb whose plants
    cross those rows at full stage-2 score; rule 8 = encodings 26 and 27, which hold most of them (6 units).  k_scan reads U as A and
    every letter outside ACGU as -4, in the f16 and in the integer main pass; the separate stage-1 pass that such a query switches
    on for every unit must leave the track alone."""
    rna, dna = helpers.dirty_case(700)
    p = mod.default_params(rule=8, strand=0)
    want, top = expected_tracks(rna, dna, p)
    as_t, _ = expected_tracks(rna.replace(b"U", b"T"), dna, p)
    print("largest column maximum per class:", top, "; values that change when U is read as T:", int((as_t != want).sum()))
    assert max(top) >= 150 and (as_t != want).sum() > 1000
    for f16 in (1, 0):
        t = _track(mod, rna, dna, p, dp_f16=f16)
        assert (t.bin, t.nbins, t.units, t.saturated_units) == (1, len(dna), 6, 0)
        _same(t.array(), want, f"dp_f16 {f16}")
