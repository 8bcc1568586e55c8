"""Panels of short oligos on the GPU (fasim_scan_oligos, k_scan_short, `fasim --oligos`): exact equality of tracks and site arrays
with the numpy restatement (test_track_cpu.py / test_sites_cpu.py, which never call the code under test) over the length edges
1 .. 112 nt and the segment edges; the reference's own column maxima (the oracle's pre_align) for oligos of at most 29 nt, where
nothing has to be left out; batches, workers, shards, resident DNA, panel order; composition with the lncRNA calls; the CLI.
GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import enabled_encodings, expected_tracks, same_seq
from test_sites_cpu import expected_potential, sites_from
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")
LENGTHS = (1, 2, 15, 16, 17, 20, 29, 31, 32, 33, 48, 64, 100, 111, 112)


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _seq(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _engine(mod, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    if got.shape != want.shape:
        raise AssertionError((what, got.shape, want.shape))
    bad = np.argwhere(got != want)
    first = tuple(bad[0].tolist())
    raise AssertionError((what, len(bad), first, int(got[first]), int(want[first])))


def _panel(golden_dir, lengths=LENGTHS):
    """Oligos of the given lengths cut from H19 (at different places, so that no two are prefixes of each other)."""
    h19 = _seq(golden_dir, "H19")
    return [h19[300 + 131 * k:300 + 131 * k + m] for k, m in enumerate(lengths)]


def _pre_image(tract: bytes, enc: int, rng) -> bytes:
    """DNA whose unit under `enc` reads `tract` (U as A) where the rule has a pre-image of the letter, a random base elsewhere; for a
    reversed encoding the DNA is laid down backwards."""
    pre = {}
    for base, o in zip(b"ATGC", synth.RULE_OUT[enc].encode()):
        pre.setdefault(o, []).append(base)
    out = bytearray()
    for ch in tract.upper().replace(b"U", b"A"):
        c = pre.get(ch)
        out.append(c[int(rng.integers(len(c)))] if c else b"ACGT"[int(rng.integers(4))])
    return bytes(out[::-1]) if enc & 1 else bytes(out)


def _planted_record(oligos, p, n, seed, period=97):
    """n nt of random DNA carrying, every `period` columns (every other slot behind a plant longer than the period), a gapped pre-image
    of every oligo -- half, a DNA-side insertion of 3 nt, half -- under the first forward and the first reversed enabled encoding."""
    rng = np.random.default_rng(seed)
    dna = bytearray(synth.random_dna(n, seed))
    encs = enabled_encodings(p)
    pair = (next(e for e in encs if not e & 1), next(e for e in encs if e & 1))
    pos = period
    for o in oligos:
        h = len(o) // 2
        for enc in pair:
            ins = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=3).tobytes())
            tract = _pre_image(o[:h], enc, rng) + ins + _pre_image(o[h:], enc, rng) if not enc & 1 else \
                _pre_image(o[h:], enc, rng) + ins + _pre_image(o[:h], enc, rng)
            if pos + len(tract) > n:
                break
            dna[pos:pos + len(tract)] = tract
            pos += period * ((len(tract) + period) // period)
    return bytes(dna)


# ---- 1. length edges ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(mod, golden_dir):
    """The panel of 15 lengths against a record of 5 000 nt -- one full segment, and the 100 nt of its overlap once more as the
    record's second segment -- rule 1, both strands (one unit per class); the restatement computed once."""
    oligos = _panel(golden_dir)
    p = mod.default_params(rule=1, strand=0)
    dna = _planted_record(oligos, p, 5000, 1601)
    assert mod.segment_count(len(dna), p) == 2 and len(enabled_encodings(p)) == 4
    tracks, pots = [], []
    for o in oligos:
        t, _ = expected_tracks(o, dna, p)
        P, per_enc = expected_potential(o, dna, p)
        t.setflags(write=False)
        P.setflags(write=False)
        tracks.append(t)
        pots.append((P, per_enc))
    return dict(oligos=oligos, p=p, dna=dna, tracks=tracks, pots=pots)


def test_length_edges_tracks_and_sites(mod, edges):
    oligos, p, dna = edges["oligos"], edges["p"], edges["dna"]
    assert [len(o) for o in oligos] == list(LENGTHS)
    tops = [int(t.max()) for t in edges["tracks"]]
    print("largest potential per oligo:", tops)
    assert min(tops) >= 5          # (rule 1 gives units over G, T and N only: the oligos' A and C never pair, the scores stay modest)
    e = _engine(mod)
    for which in (0, 1):
        vs = [max(1, (1 + which) * top // 3) for top in tops]
        # one call per threshold pair: every oligo has its own natural thresholds, the call takes one -> one call per oligo group
        for v in sorted(set(vs)):
            qs = [q for q in range(len(oligos)) if vs[q] == v]
            sites, tracks = e.scan_oligos([oligos[q] for q in qs], dna, p, min_value=v, track_bin=1)
            for k, q in enumerate(qs):
                P, per_enc = edges["pots"][q]
                _same(tracks[k][0].array(), edges["tracks"][q], f"track of the {LENGTHS[q]}-nt oligo")
                _same(sites[k][0].array(), sites_from(P, per_enc, v), f"sites of the {LENGTHS[q]}-nt oligo at {v}")
                assert (sites[k][0].units, tracks[k][0].units, sites[k][0].saturated_units, tracks[k][0].nbins) == (8, 8, 0, len(dna))
                assert len(sites[k][0]) >= 1
    # and the whole panel in one call, one threshold
    sites, tracks = e.scan_oligos(oligos, dna, p, min_value=20, track_bin=1)
    e.close()
    for q in range(len(oligos)):
        P, per_enc = edges["pots"][q]
        _same(tracks[q][0].array(), edges["tracks"][q], f"panel: track {q}")
        _same(sites[q][0].array(), sites_from(P, per_enc, 20), f"panel: sites {q}")


# ---- 2. segment edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4999, 5000, 5001])
def test_segment_edges(mod, golden_dir, n):
    """Records of one column up to two segments (5 001 nt: the overlap of 100 nt merged by maximum), a 20-nt and the 112-nt oligo."""
    oligos = _panel(golden_dir, (20, 112))
    p = mod.default_params(rule=1, strand=0)
    dna = _planted_record(oligos, p, 5001, 1602)[5001 - n:]          # the plants of the record's end stay
    e = _engine(mod)
    sites, tracks = e.scan_oligos(oligos, dna, p, min_value=10, track_bin=1)
    e.close()
    assert mod.segment_count(n, p) == (2 if n > 4900 else 1)
    for q, o in enumerate(oligos):
        want, _ = expected_tracks(o, dna, p)
        P, per_enc = expected_potential(o, dna, p)
        _same(tracks[q][0].array(), want, f"{n} nt, oligo {q}")
        _same(sites[q][0].array(), sites_from(P, per_enc, 10), f"{n} nt, oligo {q}")
        assert tracks[q][0].units == 4 * sum(not same_seq(dna[a:a + 5000]) for a in range(0, n, 4900))      # (a 1-nt record is one letter: skipped)


def test_the_largest_scores(mod):
    """Oligos over G and T only, which rule 1 can pair in full: a perfect pre-image of the 112-nt one scores 5 * 112 = 560, the
    largest value the kernel can meet, and gapped ones come close; a 50-nt one likewise.  Two segments."""
    rng = np.random.default_rng(1603)
    oligos = [bytes(rng.choice(np.frombuffer(b"GT", dtype=np.uint8), size=m).tobytes()) for m in (112, 50)]
    p = mod.default_params(rule=1, strand=0)
    dna = bytearray(_planted_record(oligos, p, 6000, 1604, period=397))
    for k, enc in enumerate(enabled_encodings(p)):
        dna[3000 + 300 * k:3000 + 300 * k + 112] = _pre_image(oligos[0], enc, rng)
    dna = bytes(dna)
    e = _engine(mod)
    sites, tracks = e.scan_oligos(oligos, dna, p, min_value=200, track_bin=1)
    e.close()
    for q, o in enumerate(oligos):
        P, per_enc = expected_potential(o, dna, p)
        assert P.max(axis=1).tolist() == [560] * 4 if q == 0 else P.max() > 200
        _same(tracks[q][0].array(), P, f"oligo {q}")
        _same(sites[q][0].array(), sites_from(P, per_enc, 200), f"oligo {q}")
        assert len(sites[q][0]) >= 2


# ---- 3. the reference itself ---------------------------------------------------------------------------------------------------------
def test_the_reference_column_maxima(mod, golden_dir, oracle_build):
    """A 20-nt and a 29-nt oligo, all 48 encodings, default parameters, the first real MEG3 peak records: the tracks folded from the
    reference's own maxColumn (the oracle's pre_align) equal the device's.  No unit is left out: 5 * 29 = 145 < 148."""
    orc = helpers.Oracle(oracle_build)
    oligos = _panel(golden_dir, (20, 29))
    p = mod.default_params()
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))
    dnas, nseg = [], 0
    for _, s in peaks:
        k = mod.segment_count(len(s), p)
        if nseg + k > 3:
            break
        dnas.append(s)
        nseg += k
    assert len(dnas) >= 2 and len(enabled_encodings(p)) == 48
    top = [0]

    def ref_colmax(rna, targets):
        rows = [orc.pre_align(rna, t) for t in targets]
        top[0] = max(top[0], max(max(r) for r in rows))
        return rows

    e = _engine(mod)
    _, tracks = e.scan_oligos(oligos, dnas, p, min_value=1, track_bin=1)
    e.close()
    for q, o in enumerate(oligos):
        for r, dna in enumerate(dnas):
            want, _ = expected_tracks(o, dna, p, colmax=ref_colmax)
            _same(tracks[q][r].array(), want, f"oligo {q}, record {r}")
            assert tracks[q][r].units == 48 * mod.segment_count(len(dna), p)
    print("largest reference column maximum:", top[0])
    assert 0 < top[0] < 148


# ---- 4. engine paths -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    """The 30.5 kb construction (lower case, an N run, a skipped segment, 7 segments) x a 20-nt and a 33-nt oligo, rule 1."""
    oligos = _panel(golden_dir, (20, 33))
    p = mod.default_params(rule=1, strand=0)
    dna = _chromosome_like()
    pots = [expected_potential(o, dna, p) for o in oligos]
    for P, _ in pots:
        P.setflags(write=False)
    v = 25
    want = [sites_from(P, per_enc, v, 2) for P, per_enc in pots]
    assert all(len(w) >= 3 for w in want)
    return dict(oligos=oligos, p=p, dna=dna, pots=pots, v=v, want=want)


def _check_chrom(chrom, sites, tracks, what):
    for q in range(2):
        _same(tracks[q][0].array(), chrom["pots"][q][0], f"{what}: track {q}")
        _same(sites[q][0].array(), chrom["want"][q], f"{what}: sites {q}")
        assert (sites[q][0].units, tracks[q][0].units) == (24, 24)


@pytest.mark.parametrize("options", [dict(seg_batch=1, workers=1), dict(seg_batch=1, workers=16), dict(seg_batch=3, workers=1),
                                     dict(seg_batch=3, workers=16), dict()])
def test_batches_and_workers(mod, chrom, options):
    e = _engine(mod, **options)
    sites, tracks = e.scan_oligos(chrom["oligos"], chrom["dna"], chrom["p"], min_value=chrom["v"], max_gap=2, track_bin=1)
    totals = e.last_totals
    e.close()
    _check_chrom(chrom, sites, tracks, str(options))
    assert [(t["segments"], t["segments_skipped"], t["units"]) for t in totals] == [(7, 1, 24)] * 2
    scanned = sum(min(5000, len(chrom["dna"]) - a) for a in range(0, len(chrom["dna"]), 4900) if a != 9800)      # (segment 2 is all N)
    assert [t["logical_cells"] for t in totals] == [m * scanned * 4 for m in (20, 33)]


def test_shards_resident_dna_and_panel_order(mod, chrom):
    oligos, dna, p, v = chrom["oligos"], chrom["dna"], chrom["p"], chrom["v"]
    e = _engine(mod)
    parts = [e.scan_oligos(oligos, dna, p, min_value=v, max_gap=2, track_bin=1, seg_first=a, seg_count=c) for a, c in ((0, 3), (3, -1))]
    for q, o in enumerate(oligos):
        for (a, c), (s, t) in zip(((0, 3), (3, -1)), parts):
            Pk, pk = expected_potential(o, dna, p, a, c)
            _same(t[q][0].array(), Pk, f"shard from {a}: track {q}")
            _same(s[q][0].array(), sites_from(Pk, pk, v, 2), f"shard from {a}: sites {q}")
    merged_s = [[mod.merge_sites([parts[0][0][q][0], parts[1][0][q][0]])] for q in range(2)]
    merged_t = [[mod.merge_tracks([parts[0][1][q][0], parts[1][1][q][0]])] for q in range(2)]
    _check_chrom(chrom, merged_s, merged_t, "merged shards")
    # resident DNA equals the streamed buffer
    e.load_dna(dna)
    sites, tracks = e.scan_oligos(oligos, None, p, min_value=v, max_gap=2, track_bin=1)
    _check_chrom(chrom, sites, tracks, "resident")
    # the panel in reversed order, sites only
    back = e.scan_oligos(oligos[::-1], dna, p, min_value=v, max_gap=2)
    e.close()
    assert isinstance(back, list) and len(back) == 2
    for q in range(2):
        _same(back[1 - q][0].array(), chrom["want"][q], f"reversed panel: sites {q}")


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------
def test_composition_with_the_lncrna_calls_and_refusals(mod, golden_dir, chrom):
    rna, demo = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    short = _seq(golden_dir, "h19_100")
    oligos, dna, p, v = chrom["oligos"], chrom["dna"], chrom["p"], chrom["v"]
    p40 = mod.default_params(cLength=40)
    gold = open(os.path.join(golden_dir, "demo_lg40.TFOsorted"), "rb").read()
    e = _engine(mod)
    e.set_query(rna)
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold
    sites = e.scan_oligos(oligos, dna, p, min_value=v, max_gap=2)
    _same(sites[0][0].array(), chrom["want"][0], "between two scans")
    # the engine's own query is still H19
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold
    cases = [(dict(oligos=[]), mod.E_ARG), (dict(oligos=[oligos[0], b""]), mod.E_ARG), (dict(oligos=[oligos[0], b"GA" * 56 + b"G"]), mod.E_ARG),
             (dict(min_value=0), mod.E_ARG), (dict(min_value=16384), mod.E_ARG), (dict(max_gap=-1), mod.E_ARG), (dict(track_bin=-1), mod.E_ARG),
             (dict(params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED)]
    for kw, code in cases:
        kw = dict(dict(oligos=oligos, params=p, min_value=v), **kw)
        with pytest.raises(mod.FasimError) as ei:
            e.scan_oligos(kw.pop("oligos"), dna, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
        print(ei.value)
        if code == mod.E_ARG and "oligos" in str(ei.value) and "113" in str(ei.value):
            assert "oligo 1" in str(ei.value) and "fasim_scan_records_sites" in str(ei.value)
    # both outputs NULL, through the C interface
    L, C = mod.lib(), __import__("ctypes")
    arr, lens = (C.c_char_p * 1)(oligos[0]), (C.c_int32 * 1)(len(oligos[0]))
    offs, rlens = (C.c_int64 * 1)(0), (C.c_int64 * 1)(len(dna))
    assert L.fasim_scan_oligos(e._h, arr, lens, 1, dna, offs, rlens, 1, 0, -1, C.byref(p), v, 0, None, 0, None, None) == mod.E_ARG
    # the lncRNA calls still refuse short queries
    with pytest.raises(mod.FasimError) as ei:
        e.scan_sites(dna, p, min_value=60, rnas=[short])
    assert ei.value.code == mod.E_UNSUPPORTED
    sites = e.scan_oligos(oligos, dna, p, min_value=v, max_gap=2)
    _same(sites[1][0].array(), chrom["want"][1], "after the refusals")
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold
    e.close()


# ---- 6. the CLI ----------------------------------------------------------------------------------------------------------------------
def _run(wd, *args, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_panel(mod, golden_dir, tmp_path):
    oligos = _panel(golden_dir, (20, 31, 112))
    names = ["tfo20", "tfo31", "tfo112"]
    (tmp_path / "panel.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), o) for n, o in zip(names, oligos)))
    (tmp_path / "testDNA.fa").write_bytes(open(os.path.join(golden_dir, "testDNA.fa"), "rb").read())
    demo = _seq(golden_dir, "testDNA")
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:3]
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    p = mod.default_params()
    e = _engine(mod)
    one = e.scan_oligos(oligos, demo, p, min_value=40, max_gap=3)
    many = e.scan_oligos(oligos, [s for _, s in peaks], p, min_value=40, max_gap=3)
    e.close()
    assert sum(len(s[0]) for s in one) >= 3 and sum(len(s) for row in many for s in row) >= 3
    plain = {f"hg19-{n}-testDNA-TFOsites-40": mod.sites_bed(one[q][0], "chr11", 2158478, n) for q, n in enumerate(names)}
    plain["panel-testDNA.oligos-40.tsv"] = mod.oligo_panel_tsv(names, oligos, one)
    sets = {}
    for q, n in enumerate(names):
        text = b"# fasim sites lncRNA=%s min_value=40 max_gap=3\n" % n.encode()
        for (h, _), st in zip(peaks, many[q]):
            name, chro, span = h.split("|")
            text += mod.sites_bed(st, chro, int(span.split("-")[0]), n, record_name=name, header=False)
        sets[f"{n}-recs.sites-40.bed"] = text
    sets["panel-recs.oligos-40.tsv"] = mod.oligo_panel_tsv(names, oligos, many)

    def run(out, f1, *extra):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", "panel.fa", "-O", out + "/", "--oligos", "--sites", "40", "--sites-gap", "3", *extra)
        return _files(tmp_path / out)

    assert run("plain", "testDNA.fa") == plain
    assert run("plain2", "testDNA.fa", "--devices", "0,0") == plain
    assert run("all", "recs.fa", "--all-records") == sets
    assert run("all2", "recs.fa", "--all-records", "--devices", "0,0") == sets


# ---- untidy oligos -----------------------------------------------------------------------------------------------------------------
def test_untidy_oligos(mod):
    """A panel of 40-nt oligos cut from helpers.dirty_query(700): one from its T-to-U stretch, one around an N / IUPAC letter, one in
    lower case, and a tidy one, against 5 kb planted with their gapped pre-images under rule 8 (encodings 26 and 27, under which
    every letter has a pre-image): tracks and sites against the restatement (U read as A, every other letter -4)."""
    q = helpers.dirty_query(700, helpers.DIRTY_SEEDS[700])
    (u0, _), (l0, _), _ = helpers.dirty_zones(700)
    n0 = helpers.dirty_rows(q)["N"][1]
    oligos = [q[u0 + 10:u0 + 50], q[n0 - 20:n0 + 20], q[l0 + 10:l0 + 50], q[400:440]]
    assert b"U" in oligos[0] and set(oligos[1]) & set(b"NRYnu") and oligos[2].islower() and set(oligos[3]) <= set(b"ACGT")
    p = mod.default_params(rule=8, strand=0)
    dna = _planted_record(oligos, p, 5000, 1610)
    e = _engine(mod)
    sites, tracks = e.scan_oligos(oligos, dna, p, min_value=60, track_bin=1)
    e.close()
    for k, o in enumerate(oligos):
        want, top = expected_tracks(o, dna, p)
        P, per_enc = expected_potential(o, dna, p)
        print(f"oligo {k} ({o.decode()}): largest potential per class {top}")
        assert max(top) >= 100
        _same(tracks[k][0].array(), want, f"track of oligo {k}")
        _same(sites[k][0].array(), sites_from(P, per_enc, 60), f"sites of oligo {k}")
        assert len(sites[k][0]) >= 1 and (sites[k][0].units, sites[k][0].saturated_units) == (4, 0)
