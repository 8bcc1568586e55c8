"""Histograms of the potential on the GPU (fasim_scan_records_hist, fasim_scan_oligos_hist, k_hist, `fasim --potential-hist`): exact
equality with np.bincount over the numpy restatement of the potential (expected_potential of test_sites_cpu.py on test_track_cpu.py,
which never calls the code under test) -- overlaps counted once with the maximum, record ends, cut / overlap pairs, shards and
their merges, values above HIST_LDS_BINS, saturation, batches, workers, the f16 switch, resident DNA, controls, oligos, the CLI.
Every comparison is integer equality.  GPU only."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_sites_cpu import expected_potential
from test_track_cpu import same_seq
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

BINS = 16384
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


def bincount4(P, covered=None):
    """(4, 16384) counts of a (4, n) potential over the covered positions (all of them by default)."""
    out = np.zeros((4, BINS), dtype=np.int64)
    for c in range(4):
        out[c] = np.bincount(P[c] if covered is None else P[c][covered], minlength=BINS)
    return out


def _same(h, want, what=""):
    got = h.array()
    assert got.dtype == np.int64 and got.shape == (4, BINS)
    if not np.array_equal(got, want):
        c, v = np.argwhere(got != want)[0]
        raise AssertionError((what, "class", int(c), "value", int(v), "got", int(got[c, v]), "want", int(want[c, v]),
                              "differing bins", int((got != want).sum())))


def _key(h):
    return (h.array().tolist(), h.positions, h.units, h.saturated_units, [(r, b, s, v.tolist()) for r, b, s, v in h.pending])


# ---- 1. the 30.5 kb construction, segment by segment -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    """The 30.5 kb construction x MEG3 under rule 1, both strands (7 segments, segment 2 all N, 24 units).  The restatement runs once
    per segment (seg_first = s, seg_count = 1): P of a range is the maximum over its segments, as the definition says."""
    rna, dna = _seq(golden_dir, "MEG3"), _chromosome_like()
    p = mod.default_params(rule=1, strand=0)
    step = p.cutLength - p.overlapLength
    nseg = mod.segment_count(len(dna), p)
    per_seg = []
    for s in range(nseg):
        P, _ = expected_potential(rna, dna, p, seg_first=s, seg_count=1)
        P.setflags(write=False)
        per_seg.append(P)

    def of_range(first, count):
        P = np.zeros((4, len(dna)), dtype=np.int64)
        cov = np.zeros(len(dna), dtype=bool)
        for s in range(first, first + count):
            P = np.maximum(P, per_seg[s])
            cov[s * step:s * step + p.cutLength] = True
        return P, cov

    return dict(rna=rna, dna=dna, p=p, step=step, nseg=nseg, per_seg=per_seg, of_range=of_range, P=of_range(0, nseg)[0])


def test_the_case_is_not_vacuous(chrom):
    p, step, n, P = chrom["p"], chrom["step"], len(chrom["dna"]), chrom["P"]
    assert (chrom["nseg"], step, p.cutLength, n) == (7, 4900, 5000, 30500)
    assert same_seq(chrom["dna"][2 * step:2 * step + 5000]) and not chrom["per_seg"][2].any()
    # an overlap position whose two segments disagree: adding per-segment counts would be wrong there
    differ = 0
    for s in range(1, 7):
        a = s * step
        differ += int((chrom["per_seg"][s - 1][:, a:a + 100] != chrom["per_seg"][s][:, a:a + 100]).sum())
    assert differ > 50
    # values counted right at a slice edge of the kernel (offsets 2 040 and 4 080 of a segment)
    edges = [a + k for a in range(0, n, step) for k in (2039, 2040, 4079, 4080) if a + k < n]
    assert (P[:, edges] > 0).sum() > 20
    assert int(P.max()) < 1024          # (this case stays inside the kernel's LDS histogram; case 5 leaves it)


def test_whole_record_equals_bincount(mod, chrom):
    e = _engine(mod, chrom["rna"])
    res, h, ctl = e.scan_hist(chrom["dna"], chrom["p"])
    e.close()
    assert res is None and ctl == []
    _same(h, bincount4(chrom["P"]), "whole")
    assert (h.positions, h.units, h.saturated_units, h.pending) == (30500, 24, 0, [])
    assert h.array().sum(axis=1).tolist() == [30500] * 4


# ---- 2. record lengths at every edge ------------------------------------------------------------------------------------------------------
LENGTHS = (1, 99, 100, 101, 2040, 2041, 4080, 4900, 4901, 4950, 5000, 5001, 9800, 9801, 9900)


@pytest.fixture(scope="module")
def piece(golden_dir):
    return _seq(golden_dir, "MEG3")[400:520]


def test_record_lengths_at_every_edge(mod, piece):
    p = mod.default_params(rule=1, strand=0)
    big = synth.planted_dna(sum(LENGTHS), 31, piece, every=300, min_len=20, max_len=60)
    dnas, at = [], 0
    for n in LENGTHS:
        dnas.append(big[at:at + n])
        at += n
    wants = [bincount4(expected_potential(piece, d, p)[0]) for d in dnas]
    # (a segment of one letter is skipped: the 1-nt record, the 1-nt last segments of the 4 901 and 9 801 nt records)
    units = [4 * sum(not same_seq(d[a:a + p.cutLength]) for a in range(0, len(d), p.cutLength - p.overlapLength)) for d in dnas]
    assert units[0] == 0 and units[LENGTHS.index(4901)] == 4 and units[LENGTHS.index(9900)] == 12
    e = _engine(mod, piece)
    _, h, _ = e.scan_hist(dnas, p)
    _same(h, sum(wants), "the set")
    assert h.positions == sum(LENGTHS) and not h.pending
    assert h.units == sum(units)
    for n, d, w, u in zip(LENGTHS, dnas, wants, units):
        _, h, _ = e.scan_hist([d], p)
        _same(h, w, f"record of {n} nt")
        assert (h.positions, h.units, h.pending) == (n, u, [])
    e.close()


# ---- 3. cut and overlap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut,ovl", [(5000, 0), (2040, 8), (2041, 1020), (300, 150)])
def test_cut_and_overlap(mod, piece, cut, ovl):
    p = mod.default_params(rule=1, strand=0, cutLength=cut, overlapLength=ovl)
    dna = bytearray(synth.planted_dna(6100, 32, piece, every=200, min_len=20, max_len=60))
    dna[900:1900] = b"N" * 1000                                       # whole skipped segments for the short cuts
    dna = bytes(dna)
    P, _ = expected_potential(piece, dna, p)
    e = _engine(mod, piece)
    _, h, _ = e.scan_hist(dna, p)
    e.close()
    _same(h, bincount4(P), f"-c {cut} -o {ovl}")
    skipped = sum(same_seq(dna[a:a + cut]) for a in range(0, len(dna), cut - ovl))
    assert (cut != 300) or skipped >= 4
    assert (h.positions, h.units, h.pending) == (len(dna), 4 * (mod.segment_count(len(dna), p) - skipped), [])


def test_overlap_above_half_the_cut_is_refused(mod, piece):
    e = _engine(mod, piece)
    dna = synth.random_dna(1000, 5)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_hist(dna, mod.default_params(rule=1, strand=0, cutLength=301, overlapLength=151))
    assert ei.value.code == mod.E_UNSUPPORTED
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_hist([b"GGAGGAGGGAAGGAGGGAGG"], dna, mod.default_params(rule=1, strand=0, cutLength=301, overlapLength=151))
    assert ei.value.code == mod.E_UNSUPPORTED
    p = mod.default_params(rule=1, strand=0, cutLength=300, overlapLength=150)
    _, h, _ = e.scan_hist(dna, p)                                     # the engine is usable afterwards
    e.close()
    _same(h, bincount4(expected_potential(piece, dna, p)[0]), "after the refusal")


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------------
def test_shards_and_their_merges(mod, chrom):
    e = _engine(mod, chrom["rna"])
    nseg, step = chrom["nseg"], chrom["step"]
    _, whole, _ = e.scan_hist(chrom["dna"], chrom["p"])
    shard = {}

    def get(first, count):
        if (first, count) not in shard:
            _, h, _ = e.scan_hist(chrom["dna"], chrom["p"], seg_first=first, seg_count=count)
            P, cov = chrom["of_range"](first, count)
            _same(h, bincount4(P, cov), f"shard {first}+{count}")
            assert h.positions == int(cov.sum()) and h.units == 4 * sum(1 for s in range(first, first + count) if s != 2)
            want_edges = ([(0, first - 1, 1)] if first > 0 else []) + ([(0, first + count - 1, 0)] if first + count < nseg else [])
            assert [(r, b, s) for r, b, s, _ in h.pending] == want_edges
            for r, b, s, v in h.pending:
                a = (b + 1) * step
                assert np.array_equal(v, P[:, a:a + 100]), (first, count, b, s)
            shard[(first, count)] = h
        return shard[(first, count)]

    for k in range(1, nseg):                                          # (k = 2 and k = 3 cut beside the all-N segment)
        a, b = get(0, k), get(k, nseg - k)
        assert _key(mod.merge_hists([a, b])) == _key(whole) == _key(mod.merge_hists([b, a])), k
    for i, j in ((1, 2), (2, 3), (2, 5), (3, 6), (1, 6)):
        parts = [get(0, i), get(i, j - i), get(j, nseg - j)]
        for perm in itertools.permutations(range(3)):
            x, y, z = (parts[t] for t in perm)
            assert _key(mod.merge_hists([x, y, z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_hists([mod.merge_hists([x, y]), z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_hists([x, mod.merge_hists([y, z])])) == _key(whole), (i, j, perm)
    e.close()


# ---- 5. values above HIST_LDS_BINS, saturation ------------------------------------------------------------------------------------------
def test_values_above_the_lds_histogram(mod, golden_dir):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dna = synth.planted_dna(5000, 41, rna, min_len=1300, max_len=1300, mut_pct=0, indel_pct=0)
    P, _ = expected_potential(rna, dna, p)
    top = int(P.max())
    print("top value", top, "positions at or above HIST_LDS_BINS", int((P >= mod.HIST_LDS_BINS).sum()))
    assert top > mod.HIST_LDS_BINS
    e = _engine(mod, rna)
    _, h, _ = e.scan_hist(dna, p)
    e.close()
    _same(h, bincount4(P), "planted copy")
    assert (h.positions, h.units, h.saturated_units) == (5000, 2 * 48, 0)          # (two segments: 5 000 nt and the 100 nt of the overlap)


def test_saturated_units(mod, golden_dir):
    """Against the unchanged scan_track(bin = 1) (too slow to restate).  The sat5k fixture saturates k_scan's doubled lanes in the
    stage-1 score of a unit (19 905), not in the stage-2 column maxima the potential is made of: its track tops out at 10 977 and
    has no saturated unit, so it checks equality only.  A count in bin 16 383 comes from a perfect copy of 3 400 nt of MALAT1
    (5 x 3 400 = 17 000 > 16 383) planted with the project's helper."""
    p = mod.default_params()
    rna, dna = _seq(golden_dir, "satq"), _seq(golden_dir, "sat5k")
    e = _engine(mod, rna)
    _, t = e.scan_track(dna, p, bin=1, records=False)
    _, h, _ = e.scan_hist(dna, p)
    track = t.array().astype(np.int64)
    print("sat5k: largest potential", int(track.max()), "saturated units", t.saturated_units)
    _same(h, bincount4(track), "sat5k")
    assert (h.saturated_units, h.units, h.positions) == (t.saturated_units, t.units, len(dna))
    rna = _seq(golden_dir, "MALAT1")
    dna = synth.planted_dna(5000, 65, rna, min_len=3400, max_len=3400, mut_pct=0, indel_pct=0)      # (seed 65: an encoding with a pre-image for every letter)
    e.set_query(rna)
    _, t = e.scan_track(dna, p, bin=1, records=False)
    _, h, _ = e.scan_hist(dna, p)
    e.close()
    track = t.array().astype(np.int64)
    assert int(track.max()) == 16383 and t.saturated_units >= 1
    _same(h, bincount4(track), "planted 3 400 nt of MALAT1")
    assert h.array()[:, 16383].sum() == int((track == 16383).sum()) > 0
    assert (h.saturated_units, h.units, h.positions) == (t.saturated_units, t.units, len(dna))


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------------
def test_batches_workers_f16_resident_and_records(mod, chrom):
    want = bincount4(chrom["P"])
    for options in (dict(workers=1), dict(workers=3, seg_batch=1), dict(seg_batch=2), dict(seg_batch=3, dp_f16=0), dict(dp_f16=1, workers=2, seg_batch=4)):
        e = _engine(mod, chrom["rna"], **options)
        _, h, _ = e.scan_hist(chrom["dna"], chrom["p"])
        _same(h, want, str(options))
        assert (h.positions, h.units, h.pending) == (30500, 24, [])
        e.close()
    e = _engine(mod, chrom["rna"], seg_batch=2)
    e.load_dna(chrom["dna"])
    _, h, _ = e.scan_hist(None, chrom["p"])
    _same(h, want, "resident")
    plain = e.scan_records([chrom["dna"]], chrom["p"])
    res, h, _ = e.scan_hist(chrom["dna"], chrom["p"], records=True)
    _same(h, want, "with stage 3")
    x, y = res[0], plain[0]
    assert y.count > 0 and (x.count, x.recs, x.pool) == (y.count, y.recs, y.pool) and [x.stats[k] for k in SEVEN] == [y.stats[k] for k in SEVEN]
    e.close()


# ---- 7. controls -------------------------------------------------------------------------------------------------------------------------
def test_controls_are_plain_queries(mod, chrom, golden_dir):
    rna = chrom["rna"]
    dna, p = chrom["dna"][:9000], chrom["p"]
    e = _engine(mod, rna)
    _, h, ctl = e.scan_hist(dna, p, controls=3, seed=7)
    assert len(ctl) == 3 and e.m == len(rna)
    _, alone, none = e.scan_hist(dna, p)
    assert _key(h) == _key(alone) and none == []
    shuffled = [mod.shuffle_query(rna, 7, k) for k in (1, 2, 3)]
    assert len(set(shuffled)) == 3 and all(sorted(s) == sorted(rna) for s in shuffled)
    for k, s in enumerate(shuffled):
        e.set_query(s)
        _, plain, _ = e.scan_hist(dna, p)
        assert _key(ctl[k]) == _key(plain), k
    _same(ctl[0], bincount4(expected_potential(shuffled[0], dna, p)[0]), "control 1 against the restatement")
    # several lncRNAs, each with its own controls; with stage 3 for the lncRNAs
    other = _seq(golden_dir, "H19")[:700]
    res, hs, cs = e.scan_hist(dna, p, controls=2, seed=9, rnas=[rna, other], records=True)
    assert len(hs) == 2 and [len(c) for c in cs] == [2, 2] and len(res) == 2 and _key(hs[0]) == _key(alone)
    for q, r in enumerate((rna, other)):
        for k in (1, 2):
            e.set_query(mod.shuffle_query(r, 9, k))
            assert _key(cs[q][k - 1]) == _key(e.scan_hist(dna, p)[1]), (q, k)
    e.close()
    assert mod.hist_threshold(h, ctl, 0.05) >= 0 and mod.hist_tsv(h, "MEG3", ctl, seed=7).startswith(b"# fasim potential histogram lncRNA=MEG3 positions=9000 controls=3 seed=7 fdr=0.05 min_value=")


# ---- 8. oligos ---------------------------------------------------------------------------------------------------------------------------
def test_oligo_panels(mod, golden_dir):
    meg3 = _seq(golden_dir, "MEG3")
    oligos = [meg3[700:701], meg3[700:720], meg3[700:812]]
    assert [len(o) for o in oligos] == [1, 20, 112]
    p = mod.default_params(rule=1, strand=0)
    dnas = [synth.planted_dna(9950, 51, meg3[690:830], every=250, min_len=18, max_len=110), synth.random_dna(4950, 52)]
    e = _engine(mod)
    hs = e.scan_oligos_hist(oligos, dnas, p)
    _, tracks = e.scan_oligos(oligos, dnas, p, min_value=1, track_bin=1)
    for q, o in enumerate(oligos):
        want = sum(bincount4(t.array().astype(np.int64)) for t in tracks[q])
        _same(hs[q], want, f"{len(o)}-nt oligo against its tracks")
        assert (hs[q].positions, hs[q].units, hs[q].pending) == (9950 + 4950, sum(t.units for t in tracks[q]), [])
    _same(hs[1], sum(bincount4(expected_potential(oligos[1], d, p)[0]) for d in dnas), "20-nt oligo against the restatement")
    # shards of a panel merge like those of a lncRNA
    parts = [e.scan_oligos_hist(oligos, dnas, p, seg_first=a, seg_count=n) for a, n in ((0, 2), (2, 1), (3, 2))]
    for q in range(3):
        assert _key(mod.merge_hists([x[q] for x in parts])) == _key(hs[q]), q
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_hist([meg3[:113]], dnas, p)
    assert ei.value.code == mod.E_ARG
    e.close()


# ---- 9. the CLI --------------------------------------------------------------------------------------------------------------------------
def _run(wd, *args, env=None, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_plain_run_and_refusals(mod, golden_dir, tmp_path):
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params(cLength=40)
    e = _engine(mod, rna)
    _, h, ctl = e.scan_hist(dna, p, controls=2, seed=5)
    e.close()
    want0, want2 = mod.hist_tsv(h, "H19"), mod.hist_tsv(h, "H19", ctl, seed=5, fdr=0.2)
    assert want0.startswith(b"# fasim potential histogram lncRNA=H19 positions=%d\nvalue\t" % len(dna)) and want0.count(b"\n") > 50
    assert b" controls=2 seed=5 fdr=0.2 min_value=" in want2.splitlines()[0] and want2.splitlines()[1].endswith(b"\tall_ge\tall_ctl_ge\tfdr")
    three = {"hg19-H19-testDNA-TFOsorted": "demo_lg40.TFOsorted", "hg19-H19-testDNA-TFOclass1-15-40": "demo_lg40.TFOclass1",
             "hg19-H19-testDNA-TFOclass2-15-40": "demo_lg40.TFOclass2"}
    gold = {n: open(os.path.join(golden_dir, f), "rb").read() for n, f in three.items()}
    name = "hg19-H19-testDNA-TFOhist"

    def run(out, *extra, status=0):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra, status=status)
        return _files(tmp_path / out)

    ctl_args = ("--hist-controls", "2", "--hist-seed", "5", "--hist-fdr", "0.2")
    assert run("full", "--potential-hist") == dict(gold, **{name: want0})
    assert run("ctl", "--potential-hist", *ctl_args) == dict(gold, **{name: want2})
    assert run("only", "--potential-hist", "--potential-hist-only") == {name: want0}
    assert run("two", "--potential-hist", "--potential-hist-only", *ctl_args, "--devices", "0,0") == {name: want2}
    refused = (["--potential-hist", "-F"], ["--potential-hist", "--accumulate-records"], ["--potential-hist", "--track", "25"],
               ["--potential-hist", "--all-records", "--screen"], ["--potential-hist", "--tfo-profile"], ["--potential-hist", "--sites", "100"],
               ["--hist-controls", "2"], ["--hist-seed", "1"], ["--hist-fdr", "0.1"], ["--potential-hist-only"],
               ["--potential-hist", "--hist-controls", "-1"], ["--potential-hist", "--hist-fdr", "0"], ["--potential-hist", "--hist-fdr", "1.01"],
               ["--potential-hist", "-c", "300", "-o", "151"], ["--oligos"])
    for k, extra in enumerate(refused):
        assert run(f"refused{k}", *extra, status=2) == {}, extra


def test_cli_record_sets_and_oligos(mod, golden_dir, tmp_path):
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:12]
    (tmp_path / "MEG3.fa").write_bytes(open(os.path.join(golden_dir, "MEG3.fa"), "rb").read())
    lnc = synth.read_fasta(str(tmp_path / "MEG3.fa"))[0]
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    e = _engine(mod, rna)
    _, h, ctl = e.scan_hist([s for _, s in peaks], p, controls=2, seed=3)
    want = mod.hist_tsv(h, lnc, ctl, seed=3)
    assert h.positions == sum(len(s) for _, s in peaks)

    def run(out, f1, f2, *extra, env=None):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", f2, "-O", out + "/", *extra, env=env)
        return _files(tmp_path / out)

    args = ("--all-records", "--potential-hist", "--hist-controls", "2", "--hist-seed", "3")
    fname = f"{lnc}-recs.hist.tsv"
    assert run("all", "recs.fa", "MEG3.fa", *args, "--potential-hist-only") == {fname: want}
    assert run("all0", "recs.fa", "MEG3.fa", *args, "--potential-hist-only", env={"FASIM_RECORD_GROUP": "0"}) == {fname: want}
    assert run("all3", "recs.fa", "MEG3.fa", *args, "--potential-hist-only", env={"FASIM_RECORD_GROUP": "3"}) == {fname: want}
    assert run("all2", "recs.fa", "MEG3.fa", *args, "--potential-hist-only", "--devices", "0,0") == {fname: want}
    plain = run("plain", "recs.fa", "MEG3.fa", "--all-records")
    assert len(plain) == 3 * len(peaks) and run("both", "recs.fa", "MEG3.fa", *args) == dict(plain, **{fname: want})
    # --regions
    g = {"chrA": b"".join(s for _, s in peaks[:4]), "chrB": b"".join(s for _, s in peaks[4:6])}
    la = len(g["chrA"])
    bed = ["chrB\t0\t4000\tchrB_head", "chrA\t1000\t5900\tlen4900", "chrA\t3000\t9000", f"chrA\t{la - 3000}\t{la}\tchrA_tail"]
    (tmp_path / "g.bed").write_text("".join(x + "\n" for x in bed))
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + g["chrA"] + b"\n>chrB some description\n" + g["chrB"] + b"\n")
    regs = mod.read_bed(tmp_path / "g.bed")
    _, h, _ = e.scan_hist([g[r.chrom][r.start:r.end] for r in regs], p)
    e.close()
    rname = f"{lnc}-genome.hist.tsv"
    assert run("reg", "genome.fa", "MEG3.fa", "--regions", "g.bed", "--potential-hist", "--potential-hist-only") == {rname: mod.hist_tsv(h, lnc)}
    assert run("reg2", "genome.fa", "MEG3.fa", "--regions", "g.bed", "--potential-hist", "--potential-hist-only", "--devices", "0,0") == {rname: mod.hist_tsv(h, lnc)}
    # --oligos
    oligos, names = [rna[700:720], rna[700:812]], ["tfo20", "tfo112"]
    (tmp_path / "panel.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), o) for n, o in zip(names, oligos)))
    e = _engine(mod)
    hs = e.scan_oligos_hist(oligos, [s for _, s in peaks], p)
    cs = [e.scan_oligos_hist([mod.shuffle_query(o, 3, k) for k in (1, 2)], [s for _, s in peaks], p) for o in oligos]
    e.close()
    wanto = {f"{n}-recs.hist.tsv": mod.hist_tsv(hs[q], n, cs[q], seed=3) for q, n in enumerate(names)}
    assert run("oligos", "recs.fa", "panel.fa", "--oligos", *args) == wanto
    assert run("oligos2", "recs.fa", "panel.fa", "--oligos", *args, "--devices", "0,0") == wanto


# ---- an untidy query ----------------------------------------------------------------------------------------------------------------
def test_untidy_query(mod):
    """helpers.dirty_case(700) (U, lower case, N R Y n u in the query) under rule 8, three segments: the histogram of the restated
    potential (U read as A, every other letter -4)."""
    rna, dna = helpers.dirty_case(700)
    p = mod.default_params(rule=8, strand=0)
    P, _ = expected_potential(rna, dna, p)
    assert int(P.max()) >= 150
    e = _engine(mod, rna)
    res, h, ctl = e.scan_hist(dna, p)
    e.close()
    assert res is None and ctl == []
    _same(h, bincount4(P), "untidy query")
    assert (h.positions, h.units, h.saturated_units, h.pending) == (len(dna), 6, 0, [])
