"""Record sets and BED intervals screened by potential on the GPU (fasim_scan_records_track, k_track's peak variants, `fasim
--screen`): tracks and peaks against the numpy restatement of test_track_cpu.py (which never calls the code under test), against
scan_track of every record alone and against scan_records; batches, workers, the f16 switch, resident DNA and shards; refusals;
the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import bin_reduce, colmax_units, enabled_encodings, enc_class, encode_unit, same_seq
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

SEVEN = ("segments", "segments_skipped", "units", "candidates", "align_calls", "logical_cells", "cells_stage2")
EXE = os.path.join(entry.PKG_DIR, "fasim")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def peaks(golden_dir):
    return helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))


def _seq(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _engine(mod, rna=None, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    if rna is not None:
        e.set_query(rna)
    return e


def expected(rna, dna, p, seg_first=0, seg_count=-1):
    """The definition (DESIGN.md sections 11 and 12) for one record, from the restatement's column maxima: P[c][x] as a (4, n)
    array, and per class the peak (max, first argmax, smallest enabled encoding of the class one of whose units covering that
    position attains the max there), (0, -1, -1) where P[c] is zero."""
    big = len(dna)
    step = p.cutLength - p.overlapLength
    starts = list(range(0, big, step))
    last = len(starts) if seg_count < 0 else min(len(starts), seg_first + seg_count)
    encs = enabled_encodings(p)
    out = np.zeros((4, big), dtype=np.int64)
    per_enc = {e: np.full(big, -1, dtype=np.int64) for e in encs}
    for a in starts[max(0, seg_first):last]:
        seg = dna[a:a + p.cutLength]
        if same_seq(seg):
            continue
        cm = colmax_units(rna, [encode_unit(seg, e) for e in encs])
        for k, e in enumerate(encs):
            row = cm[k][::-1] if e & 1 else cm[k]
            c = enc_class(e)
            out[c, a:a + len(seg)] = np.maximum(out[c, a:a + len(seg)], row)
            per_enc[e][a:a + len(seg)] = np.maximum(per_enc[e][a:a + len(seg)], row)
    pk = np.zeros((4, 3), dtype=np.int64)
    for c in range(4):
        v = int(out[c].max()) if big else 0
        if v == 0:
            pk[c] = (0, -1, -1)
            continue
        pos = int(np.argmax(out[c]))
        pk[c] = (v, pos, min(e for e in encs if enc_class(e) == c and per_enc[e][pos] == v))
    return out, pk


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), [(tuple(int(i) for i in ix), int(got[tuple(ix)]), int(want[tuple(ix)])) for ix in bad[:6]])


def _track_peaks(track):
    """(4, 3) array of (max, first argmax) of a bin = 1 track, enc column -2 (not derivable from the track)"""
    a = track.array().astype(np.int64)
    out = np.zeros((4, 2), dtype=np.int64)
    for c in range(4):
        v = int(a[c].max()) if a.shape[1] else 0
        out[c] = (v, int(np.argmax(a[c]))) if v else (0, -1)
    return out


# ---- 1. peaks against the restatement, default parameters ------------------------------------------------------------------------
def test_first_24_peaks_equal_the_restatement(mod, golden_dir, peaks):
    """24 real records x MEG3, 48 units each: the bin = 1 tracks are expected_tracks of each record, the peaks the restatement's
    (max, first argmax, smallest attaining encoding); the peaks-only call (bin = 0, no stage 3) gives the same peaks."""
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dnas = [s for _, s in peaks[:24]]
    e = _engine(mod, rna)
    res, trk, pk = e.scan_records_track(dnas, p, bin=1)
    none, no_trk, pk0 = e.scan_records_track(dnas, p, bin=0, records=False)
    e.close()
    assert none is None and no_trk is None and pk.shape == (24, 4, 3) and pk.dtype == np.int64
    ties = 0
    for r, dna in enumerate(dnas):
        want, wpk = expected(rna, dna, p)
        _same(trk[r].array(), want, f"record {r} track")
        _same(pk[r], wpk, f"record {r} peaks")
        assert (trk[r].bin, trk[r].nbins, trk[r].units) == (1, len(dna), 48)
        ties += sum(int((want[c] == want[c].max()).sum() > 1) for c in range(4))
        if r == 0:
            # ties are real: record 0 attains its class-1 and class-2 maxima at two positions each
            assert [int((want[c] == want[c].max()).sum()) for c in (1, 2)] == [2, 2]
    print(f"{ties} of 96 (record, class) pairs attain their maximum at more than one position")
    _same(pk0, pk, "peaks only")


# ---- 2. all 532 records x [MEG3, H19] ----------------------------------------------------------------------------------------------
def test_all_peaks_two_queries_equal_single_record_calls(mod, golden_dir, peaks):
    rnas = [_seq(golden_dir, "MEG3"), _seq(golden_dir, "H19")]
    p = mod.default_params()
    dnas = [s for _, s in peaks]
    assert len(dnas) == 532 and max(len(d) for d in dnas) == 4894
    e = _engine(mod)
    plain = e.scan_records(dnas, p, rnas=rnas)
    out = {b: e.scan_records_track(dnas, p, rnas=rnas, bin=b) for b in (1, 25)}
    for b, (res, trk, pk) in out.items():
        assert pk.shape == (2, 532, 4, 3)
        for q in range(2):
            for r in range(532):
                x, y = res[q][r], plain[q][r]
                assert (x.count, x.recs, x.pool) == (y.count, y.recs, y.pool), (b, q, r)
                assert [x.stats[k] for k in SEVEN] == [y.stats[k] for k in SEVEN], (b, q, r)
    _same(out[25][2], out[1][2], "peaks of bin 25 against bin 1")
    for r, dna in enumerate(dnas):
        for b in (1, 25):
            _, alone = e.scan_track(dna, p, rnas=rnas, bin=b, records=False)
            for q in range(2):
                t = out[b][1][q][r]
                assert np.array_equal(t.array(), alone[q].array()), (b, q, r)
                assert (t.bin, t.nbins, t.units, t.saturated_units) == (b, alone[q].nbins, alone[q].units, alone[q].saturated_units)
                if b == 1:
                    _same(out[1][2][q, r, :, :2], _track_peaks(t), f"query {q} record {r}: peak against its own track")
    e.close()
    pk = out[1][2]
    assert (pk[..., 0] > 0).all() and (pk[..., 2] >= 0).all()
    for c in range(4):
        assert {enc_class(int(x)) for x in pk[:, :, c, 2].ravel()} == {c}


# ---- 3. multi-segment records ---------------------------------------------------------------------------------------------------
def test_multi_segment_records_equal_the_restatement(mod, golden_dir, peaks):
    """cutLength 2 000 / overlap 100, rule 1, both strands (4 units per segment): the first 12 peaks are two segments each, and a
    peak may lie in the overlap that both cover."""
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params(cutLength=2000, overlapLength=100, rule=1, strand=0)
    dnas = [s for _, s in peaks[:12]]
    assert [mod.segment_count(len(d), p) for d in dnas] == [2] * 12
    e = _engine(mod, rna)
    res, trk, pk = e.scan_records_track(dnas, p, bin=1)
    _, trk7, pk7 = e.scan_records_track(dnas, p, bin=7, records=False)
    e.close()
    for r, dna in enumerate(dnas):
        want, wpk = expected(rna, dna, p)
        _same(trk[r].array(), want, f"record {r} track")
        _same(trk7[r].array(), bin_reduce(want, 7), f"record {r} track, bin 7")
        _same(pk[r], wpk, f"record {r} peaks")
    _same(pk7, pk, "bin 7, track only")


def _spans():
    """Overlapping, nested, repeated and out-of-order spans of the 30.5 kb construction; (10 000, 14 500) lies wholly in the N
    block [9 800, 14 800)."""
    return [(15000, 30500), (0, 9000), (2000, 3000), (10000, 14500), (0, 9000), (4000, 16000), (20010, 20030), (30499, 30500),
            (100, 5001)]


def test_regions_of_a_chromosome_equal_the_restatement(mod, golden_dir):
    rna, dna = _seq(golden_dir, "MEG3"), _chromosome_like()
    p = mod.default_params(rule=1, strand=0)
    spans = _spans()
    e = _engine(mod, rna)
    res, trk, pk = e.scan_regions_track(dna, spans, p, bin=1)
    plain = e.scan_regions(dna, spans, p)
    e.load_dna(dna)
    _, trk_r, pk_r = e.scan_regions_track(None, spans, p, bin=1, records=False)
    e.close()
    for k, (a, b) in enumerate(spans):
        want, wpk = expected(rna, dna[a:b], p)
        _same(trk[k].array(), want, f"span {k} track")
        _same(pk[k], wpk, f"span {k} peaks")
        assert np.array_equal(trk_r[k].array(), trk[k].array()), k
        assert (res[k].recs, res[k].pool) == (plain[k].recs, plain[k].pool), k
    _same(pk_r, pk, "resident")
    assert not trk[3].array().any() and pk[3].tolist() == [[0, -1, -1]] * 4
    assert trk[3].units == 0 and trk[0].units > 0
    assert pk[1].tolist() == pk[4].tolist() and pk[1][:, 0].min() > 0


# ---- 4. invariance --------------------------------------------------------------------------------------------------------------
def test_batches_workers_f16_resident_and_shards_change_nothing(mod, golden_dir, peaks):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params(cutLength=2000, overlapLength=100, rule=1, strand=0)
    dnas = [s for _, s in peaks[:12]]
    nseg = [mod.segment_count(len(d), p) for d in dnas]

    def run(bin=1, records=False, seg_first=0, seg_count=-1, resident=False, **options):
        e = _engine(mod, rna, **options)
        if resident:
            e.load_dna(b"".join(dnas))
            out = e.scan_records_track(None, p, bin=bin, records=records, seg_first=seg_first, seg_count=seg_count,
                                       rec_lens=[len(d) for d in dnas])
        else:
            out = e.scan_records_track(dnas, p, bin=bin, records=records, seg_first=seg_first, seg_count=seg_count)
        e.close()
        return out

    _, base, base_pk = run()
    base25 = run(bin=25)[1]

    def check(got, what, ref=base):
        _, trk, pk = got
        _same(pk, base_pk, what + ": peaks")
        if trk is not None:
            for r in range(len(dnas)):
                assert np.array_equal(trk[r].array(), ref[r].array()), (what, r)

    for seg_batch in (1, 3):
        for workers in (1, 16):
            check(run(seg_batch=seg_batch, workers=workers), f"seg_batch {seg_batch} workers {workers}")
            check(run(bin=25, seg_batch=seg_batch, workers=workers), f"seg_batch {seg_batch} workers {workers} bin 25", base25)
            check(run(bin=0, seg_batch=seg_batch, workers=workers), f"seg_batch {seg_batch} workers {workers} peaks only")
    for f16 in (0, 1):
        check(run(dp_f16=f16), f"dp_f16 {f16}")
        check(run(bin=0, dp_f16=f16), f"dp_f16 {f16} peaks only")
    check(run(resident=True), "resident")
    check(run(records=True), "with stage 3")
    check(run(bin=0, records=True), "peaks only with stage 3")
    # a split inside a record (between the two segments of record 5), shards merged
    assert nseg == [2] * 12
    cut = sum(nseg[:5]) + 1
    for b, ref in ((1, base), (25, base25)):
        _, ta, pa = run(bin=b, seg_first=0, seg_count=cut)
        _, tb, pb = run(bin=b, seg_first=cut)
        assert not np.array_equal(pa, base_pk) and not np.array_equal(pb, base_pk)
        _same(mod.merge_peaks([pa, pb]), base_pk, f"merged shards, bin {b}")
        _same(mod.merge_peaks([pb, pa]), base_pk, f"merged shards the other way round, bin {b}")
        for r in range(len(dnas)):
            assert np.array_equal(mod.merge_tracks([ta[r], tb[r]]).array(), ref[r].array()), (b, r)
        # records wholly in the other shard contribute nothing
        assert pa[-1].tolist() == [[0, -1, -1]] * 4 and pb[0].tolist() == [[0, -1, -1]] * 4
    _, _, p0a = run(bin=0, seg_first=0, seg_count=cut)
    _, _, p0b = run(bin=0, seg_first=cut)
    _same(mod.merge_peaks([p0a, p0b]), base_pk, "merged shards, peaks only")


# ---- 5. track-only mode ---------------------------------------------------------------------------------------------------------
def test_peaks_only_runs_no_stage_3(mod, golden_dir, peaks):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dnas = [s for _, s in peaks[24:64]]
    e = _engine(mod, rna)
    res, _, pk = e.scan_records_track(dnas, p, bin=0, records=True)
    full = dict(e.last_totals[0])
    none, trk, pk0 = e.scan_records_track(dnas, p, bin=0, records=False)
    only = dict(e.last_totals[0])
    e.close()
    assert none is None and trk is None
    assert full["align_calls"] > 0 and full["candidates"] > 0
    assert only["align_calls"] == 0 and only["kernel_launches"][2] == 0 and only["kernel_launches"][3] == 0
    assert (only["segments"], only["units"]) == (full["segments"], full["units"]) == (40, 40 * 48)
    _same(pk0, pk, "peaks only against peaks with stage 3")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mod, golden_dir, peaks):
    rna = _seq(golden_dir, "MEG3")
    dnas = [s for _, s in peaks[:3]]
    short = rna[:112]
    e = _engine(mod, rna)
    _, _, want = e.scan_records_track(dnas, bin=0, records=False)
    cases = ((dict(rnas=[short]), mod.E_UNSUPPORTED), (dict(rnas=[rna, short], bin=25), mod.E_UNSUPPORTED),
             (dict(params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED), (dict(bin=-1), mod.E_ARG),
             (dict(bin=-25, records=False), mod.E_ARG))
    for kw, code in cases:
        with pytest.raises(mod.FasimError) as ei:
            e.scan_records_track(dnas, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
        print(ei.value)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_records_track([dnas[0], b"", dnas[2]], bin=0)
    assert ei.value.code == mod.E_ARG and "record 1" in str(ei.value)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_regions_track(dnas[0], [(0, 100), (50, 50)])
    assert ei.value.code == mod.E_ARG
    _, _, again = e.scan_records_track(dnas, bin=0, records=False)
    _same(again, want, "after the refusals")
    e.set_query(short)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_records_track(dnas, bin=0)
    assert ei.value.code == mod.E_UNSUPPORTED
    e.set_query(rna)
    _same(e.scan_records_track(dnas, bin=0, records=False)[2], want, "after the short query")
    e.close()


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------
def _run(wd, *args, env=None, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_screen_tables(mod, golden_dir, peaks, tmp_path):
    g = {"chrA": b"".join(s for _, s in peaks[:4]), "chrB": b"".join(s for _, s in peaks[4:6])}
    la, lb = len(g["chrA"]), len(g["chrB"])
    bed = [f"chrB\t0\t4000\tchrB_head", f"chrA\t1000\t5900\tlen4900", f"chrA\t3000\t9000", f"chrA\t3500\t4200\tinner",
           f"chrA\t{la - 3000}\t{la}\tchrA_tail", f"chrA\t1000\t5900\tlen4900", f"chrB\t{lb - 1}\t{lb}", f"chrA\t100\t2100\tdup",
           f"chrB\t100\t2100\tdup"]
    (tmp_path / "g.bed").write_text("".join(x + "\n" for x in bed))
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + g["chrA"] + b"\n>chrB some description\n" + g["chrB"] + b"\n")
    for f in ("MEG3.fa", "H19.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    (tmp_path / "two.fa").write_bytes((tmp_path / "MEG3.fa").read_bytes().rstrip(b"\n") + b"\n" + (tmp_path / "H19.fa").read_bytes())
    names = [synth.read_fasta(str(tmp_path / f))[0] for f in ("MEG3.fa", "H19.fa")]
    rnas = [_seq(golden_dir, "MEG3"), _seq(golden_dir, "H19")]
    p = mod.default_params()
    regs = mod.read_bed(tmp_path / "g.bed")
    assert len(regs) == len(bed)
    e = _engine(mod)
    _, _, pk = e.scan_records_track([g[r.chrom][r.start:r.end] for r in regs], p, rnas=rnas, bin=0, records=False)
    e.close()
    segs = [mod.segment_count(r.end - r.start, p) for r in regs]
    want = {f"{names[q]}-genome.screen.tsv": mod.screen_tsv(regs, segs, pk[q]) for q in range(2)}
    assert max(segs) == 2 and all(len(t.splitlines()) == 1 + len(bed) for t in want.values())

    def run(out, *extra, env=None):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "genome.fa", "-f2", "two.fa", "-O", out + "/", *extra, env=env)
        return _files(tmp_path / out)

    only = run("only", "--regions", "g.bed", "--screen-only")
    assert only == want
    assert run("only2", "--regions", "g.bed", "--screen-only", "--devices", "0,0") == want
    assert run("only1", "--regions", "g.bed", "--screen-only", env={"FASIM_RECORD_GROUP": "0"}) == want
    assert run("only3", "--regions", "g.bed", "--screen-only", env={"FASIM_RECORD_GROUP": "3"}) == want
    plain = run("plain", "--regions", "g.bed")
    assert len(plain) == 2 * (3 * len(bed) + 1)
    both = run("both", "--regions", "g.bed", "--screen")
    assert both == dict(plain, **want)
    assert run("both2", "--regions", "g.bed", "--screen", "--devices", "0,0") == both

    # --all-records: one line per record, `line` = its 1-based ordinal; grouped tracks equal one scan per record
    fa = b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks[6:12])
    (tmp_path / "recs.fa").write_bytes(fa)
    rows = []
    for k, (h, s) in enumerate(peaks[6:12]):
        name, chro, span = h.split("|")
        a = int(span.split("-")[0])
        rows.append(mod.Region(k + 1, chro, a - 1, a - 1 + len(s), name))
    e = _engine(mod, rnas[0])
    _, _, pk = e.scan_records_track([s for _, s in peaks[6:12]], p, bin=0, records=False)
    e.close()
    want_all = mod.screen_tsv(rows, [1] * 6, pk)

    def run_all(out, *extra, env=None):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "recs.fa", "-f2", "MEG3.fa", "-O", out + "/", "--all-records", *extra, env=env)
        return _files(tmp_path / out)

    assert run_all("all_only", "--screen-only") == {f"{names[0]}-recs.screen.tsv": want_all}
    grouped = run_all("trk_grouped", "--track", "25")
    alone = run_all("trk_alone", "--track", "25", env={"FASIM_RECORD_GROUP": "0"})
    assert len(alone) == 6 * 4 and grouped == alone
    assert sum(n.endswith("-TFOpotential-25") for n in alone) == 6
    assert run_all("trk_two", "--track", "25", "--devices", "0,0") == alone
    assert run_all("trk_only", "--track", "25", "--track-only") == {n: t for n, t in alone.items() if n.endswith("-TFOpotential-25")}
    scr = run_all("trk_screen", "--track", "25", "--screen")
    assert scr == dict(alone, **{f"{names[0]}-recs.screen.tsv": want_all})
