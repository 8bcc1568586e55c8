"""Per-base profiles and peaks of oligo panels on the GPU (fasim_scan_oligos_profile, fasim_scan_oligos_peaks, k_scan_short_rows,
k_rowfold_parts, `fasim --oligos --oligo-profile / --oligo-screen`): exact equality with the numpy restatement
(test_tfo_profile_cpu.py / test_sites_cpu.py, which never call the code under test) over the length edges 1 .. 112 nt, the segment
edges, hits that end on a segment's last base (where a column of code N behind the unit would raise a row), stretches, batches,
workers, record sets, shards, resident DNA, panel order, untidy oligos; the peaks; composition with the lncRNA calls; the CLI.
GPU only."""
import ctypes
import os

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import enabled_encodings, encode_unit, same_seq
from test_sites_cpu import expected_potential
from test_tfo_profile_cpu import expected_profile, expected_profiles, rowmax_units
from test_gpu_track import _chromosome_like
from test_gpu_oligos import LENGTHS, _files, _panel, _planted_record, _pre_image, _run, _same, _seq, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _gt(rng, m):
    """An oligo over G and T only, which rule 1 can pair in full."""
    return bytes(rng.choice(np.frombuffer(b"GT", dtype=np.uint8), size=m).tobytes())


def _check(prof, want, units, what):
    _same(prof.array(), want, what)
    assert (prof.m, prof.units, prof.saturated_units) == (want.shape[1], units, 0), (what, prof.m, prof.units, prof.saturated_units)


def peaks_from(P, per_enc, p):
    """The (max, first argmax, smallest encoding) rule of test_gpu_screen.expected on the two halves expected_potential returns."""
    from test_track_cpu import enc_class
    pk = np.zeros((4, 3), dtype=np.int64)
    for c in range(4):
        v = int(P[c].max()) if P.shape[1] else 0
        if v == 0:
            pk[c] = (0, -1, -1)
            continue
        pos = int(np.argmax(P[c]))
        pk[c] = (v, pos, min(e for e in enabled_encodings(p) if enc_class(e) == c and per_enc[e][pos] == v))
    return pk


# ---- 1. length edges ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(mod):
    rng = np.random.default_rng(2501)
    oligos = [_gt(rng, m) for m in LENGTHS]
    p = mod.default_params(rule=1, strand=0)
    dna = _planted_record(oligos, p, 5000, 2502)
    assert mod.segment_count(len(dna), p) == 2 and len(enabled_encodings(p)) == 4
    want = []
    for o in oligos:
        w, units = expected_profile(o, [dna], p)
        assert units == 8
        w.setflags(write=False)
        want.append(w)
    return dict(oligos=oligos, p=p, dna=dna, want=want)


def test_length_edges(mod, edges):
    oligos, p, dna, want = edges["oligos"], edges["p"], edges["dna"], edges["want"]
    for o, w in zip(oligos, want):          # no vacuous pass: every row of every class is reached, the planted halves in full
        m = len(o)
        assert w.shape == (4, m) and w.min() > 0, (m, w.min(axis=1))
        assert min(int(w[0].max()), int(w[1].max())) >= 5 * (m - m // 2), (m, w.max(axis=1))
    e = _engine(mod)
    for q, o in enumerate(oligos):
        (prof,) = e.scan_oligos_profile([o], dna, p)
        _check(prof, want[q], 8, f"alone: the {len(o)}-nt oligo")
    panel = e.scan_oligos_profile(oligos, dna, p)
    _, tracks = e.scan_oligos(oligos, dna, p, min_value=1, track_bin=1)
    e.close()
    assert len(panel) == len(oligos)
    for q, o in enumerate(oligos):
        _check(panel[q], want[q], 8, f"panel: the {len(o)}-nt oligo")
        # fact 1 of section 13: the largest row maximum is the largest column maximum, class by class
        assert panel[q].array().max(axis=1).tolist() == tracks[q][0].array().max(axis=1).tolist(), len(o)


# ---- 2. segment edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4999, 5000, 5001])
def test_segment_edges(mod, golden_dir, n):
    """Records of one column up to two segments; 5 001 nt gives a second segment of 101 nt in which most stretch pairs are void: their
    lanes return before they write, and the fold must not read their parts."""
    oligos = _panel(golden_dir, (20, 112))
    p = mod.default_params(rule=1, strand=0)
    dna = _planted_record(oligos, p, 5001, 1602)[5001 - n:]
    e = _engine(mod)
    # (a longer scan first, so that a part which is not written would hold an earlier oligo's values, not zeros)
    e.scan_oligos_profile(oligos[::-1], _planted_record(oligos, p, 5001, 1602), p)
    profs = e.scan_oligos_profile(oligos, dna, p)
    e.close()
    units = 4 * sum(not same_seq(dna[a:a + 5000]) for a in range(0, n, 4900))
    for q, o in enumerate(oligos):
        want, u = expected_profile(o, [dna], p)
        assert u == units
        _check(profs[q], want, units, f"{n} nt, oligo {q}")


# ---- 3. a hit that ends on a segment's last base ---------------------------------------------------------------------------------------
def _ends_cases(o, p, rng):
    """[(record, seg_count, (the unit the plant ends, its encoding))]: the pre-image of the oligo's first 3 m / 5 letters as a hit that
    ends on the last column of its unit -- under the first forward enabled encoding at the end of a full 5 000-nt segment (only that
    segment is scanned: the next one would hold the plant in its middle, and its row), at the end of a short last segment whose length
    is no multiple of 16 and of one whose length is, and under the first reversed encoding at the record's start."""
    encs = enabled_encodings(p)
    fwd, rev = next(e for e in encs if not e & 1), next(e for e in encs if e & 1)
    k = 3 * len(o) // 5
    out = []
    for n, at, enc, count in ((4900 + 1237, 5000 - k, fwd, 1), (4900 + 1237, 4900 + 1237 - k, fwd, -1), (4900 + 1232, 4900 + 1232 - k, fwd, -1),
                              (4900 + 1237, 0, rev, -1)):
        dna = bytearray(synth.random_dna(n, int(rng.integers(1 << 30))))
        dna[at:at + k] = _pre_image(o[:k], enc, rng)
        dna = bytes(dna)
        out.append((dna, count, (dna[0:5000] if at < 5000 else dna[4900:], enc)))
    return out


@pytest.mark.parametrize("m", [20, 33, 112])
def test_a_hit_that_ends_on_the_last_base(mod, golden_dir, m):
    """Rule 8 (encodings 26 and 27, under which every letter has a pre-image), an oligo cut from H19."""
    rng = np.random.default_rng(2530 + m)
    (o,) = _panel(golden_dir, (m,))
    p = mod.default_params(rule=8, strand=0)
    k = 3 * m // 5
    cases = _ends_cases(o, p, rng)
    for dna, _, (seg, enc) in cases:
        u = encode_unit(seg, enc)
        _, plain = rowmax_units(o, [u])
        _, drained = rowmax_units(o, [u + b"N"])
        # the inputs bite: one column of code N behind the unit raises row 3 m / 5 to 5 * (3 m / 5) - 4
        assert int(drained[0][k]) == 5 * k - 4 > int(plain[0][k]), (m, len(dna), enc, int(plain[0][k]), int(drained[0][k]))
    e = _engine(mod)
    for dna, count, (_, enc) in cases:
        want, units = expected_profile(o, [dna], p, 0, count)
        (prof,) = e.scan_oligos_profile([o], dna, p, seg_count=count)
        _check(prof, want, units, f"{m} nt, record of {len(dna)} nt, encoding {enc}, {count} segments")
    e.close()


# ---- 4. stretches, batches, workers ----------------------------------------------------------------------------------------------------
def _plant_every(dna, oligos, p, seed, period=97):
    """Gapped pre-images of the oligos (_planted_record's) every `period` columns of an existing record, under the first forward and
    the first reversed enabled encoding in turn; runs of N stay as they are."""
    rng = np.random.default_rng(seed)
    dna = bytearray(dna)
    encs = enabled_encodings(p)
    pair = (next(e for e in encs if not e & 1), next(e for e in encs if e & 1))
    for k, pos in enumerate(range(period, len(dna) - 2 * period, period)):
        o, enc = oligos[k % len(oligos)], pair[(k // len(oligos)) % 2]
        h = len(o) // 2
        ins = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=3).tobytes())
        tract = _pre_image(o[:h], enc, rng) + ins + _pre_image(o[h:], enc, rng) if not enc & 1 else \
            _pre_image(o[h:], enc, rng) + ins + _pre_image(o[:h], enc, rng)
        if b"N" in bytes(dna[pos - 1:pos + len(tract) + 1]):
            continue
        dna[pos:pos + len(tract)] = tract
    return bytes(dna)


@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    """The 30.5 kb construction (lower case, an N run, a skipped segment, 7 segments) planted every 97 columns, so that hits cross every
    stretch border, x a 20-nt and a 33-nt oligo, rule 1."""
    oligos = _panel(golden_dir, (20, 33))
    p = mod.default_params(rule=1, strand=0)
    dna = _plant_every(_chromosome_like(), oligos, p, 2540)
    assert same_seq(dna[9800:14800]) and mod.segment_count(len(dna), p) == 7
    want = []
    for o in oligos:
        w, units = expected_profile(o, [dna], p)
        assert units == 24 and w.max() >= 40
        w.setflags(write=False)
        want.append(w)
    pots = [expected_potential(o, dna, p) for o in oligos]
    return dict(oligos=oligos, p=p, dna=dna, want=want, pots=pots)


@pytest.mark.parametrize("options", [dict(seg_batch=1, workers=1), dict(seg_batch=1, workers=16), dict(seg_batch=3, workers=1),
                                     dict(seg_batch=3, workers=16), dict()])
def test_stretches_batches_and_workers(mod, chrom, options):
    e = _engine(mod, **options)
    profs = e.scan_oligos_profile(chrom["oligos"], chrom["dna"], chrom["p"])
    totals = e.last_totals
    e.close()
    for q in range(2):
        _check(profs[q], chrom["want"][q], 24, f"{options}: oligo {q}")          # (24 units: the all-N segment contributes nothing)
    assert [(t["segments"], t["segments_skipped"], t["units"]) for t in totals] == [(7, 1, 24)] * 2


# ---- 5. record sets ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recset(mod, golden_dir):
    """The first three MEG3 peaks, a record of 1 nt and one of A only (both skipped by the same-letter rule) x a 20-nt and a 48-nt
    oligo, default parameters: 48 encodings, twelve per class."""
    oligos = _panel(golden_dir, (20, 48))
    p = mod.default_params()
    dnas = [s for _, s in helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:3]] + [b"G", b"A" * 300]
    per = [expected_profiles(o, dnas, p) for o in oligos]
    pots = [[expected_potential(o, d, p) for d in dnas] for o in oligos]
    return dict(oligos=oligos, p=p, dnas=dnas, per=per, pots=pots)


def test_record_sets(mod, recset):
    oligos, p, dnas = recset["oligos"], recset["p"], recset["dnas"]
    nseg = [mod.segment_count(len(d), p) for d in dnas]
    units = [48 * k for k in nseg[:3]] + [0, 0]
    e = _engine(mod)
    per = e.scan_oligos_profile(oligos, dnas, p, per_record=True)
    whole = e.scan_oligos_profile(oligos, dnas, p)
    for q, o in enumerate(oligos):
        want, total = recset["per"][q]
        assert total == sum(units) and len(per[q]) == len(dnas)
        for r, d in enumerate(dnas):
            _check(per[q][r], want[r], units[r], f"oligo {q}, record {r}")
            (alone,) = e.scan_oligos_profile([o], d, p)
            _check(alone, want[r], units[r], f"oligo {q}, record {r} alone")
        assert want[0].max() > 0 and not want[3].any() and not want[4].any()
        _check(whole[q], np.maximum.reduce(want), sum(units), f"oligo {q}, the whole set")
    e.close()


# ---- 6. shards, resident DNA, panel order --------------------------------------------------------------------------------------------
def test_shards_resident_dna_and_panel_order(mod, chrom):
    oligos, dna, p = chrom["oligos"], chrom["dna"], chrom["p"]
    e = _engine(mod)
    parts = [e.scan_oligos_profile(oligos, dna, p, seg_first=a, seg_count=c) for a, c in ((0, 3), (3, -1))]
    for q, o in enumerate(oligos):
        for (a, c), part in zip(((0, 3), (3, -1)), parts):
            want, units = expected_profile(o, [dna], p, a, c)
            _check(part[q], want, units, f"shard from {a}: oligo {q}")
        _check(mod.merge_tfo_profiles([parts[0][q], parts[1][q]]), chrom["want"][q], 24, f"merged shards: oligo {q}")
    e.load_dna(dna)
    for q, prof in enumerate(e.scan_oligos_profile(oligos, None, p)):
        _check(prof, chrom["want"][q], 24, f"resident: oligo {q}")
    back = e.scan_oligos_profile(oligos[::-1], dna, p)
    e.close()
    for q in range(2):
        _check(back[1 - q], chrom["want"][q], 24, f"reversed panel: oligo {q}")


# ---- 7. untidy oligos ----------------------------------------------------------------------------------------------------------------
def test_untidy_oligos(mod):
    """The four 40-nt oligos of test_gpu_oligos.test_untidy_oligos (U, N / IUPAC, lower case, tidy) under rule 8."""
    q = helpers.dirty_query(700, helpers.DIRTY_SEEDS[700])
    (u0, _), (l0, _), _ = helpers.dirty_zones(700)
    n0 = helpers.dirty_rows(q)["N"][1]
    oligos = [q[u0 + 10:u0 + 50], q[n0 - 20:n0 + 20], q[l0 + 10:l0 + 50], q[400:440]]
    assert b"U" in oligos[0] and set(oligos[1]) & set(b"NRYnu") and oligos[2].islower() and set(oligos[3]) <= set(b"ACGT")
    p = mod.default_params(rule=8, strand=0)
    dna = _planted_record(oligos, p, 5000, 1610)
    e = _engine(mod)
    profs = e.scan_oligos_profile(oligos, dna, p)
    e.close()
    for k, o in enumerate(oligos):
        want, units = expected_profile(o, [dna], p)
        assert want.max() >= 100
        _check(profs[k], want, units, f"oligo {k}")


# ---- 8. peaks ------------------------------------------------------------------------------------------------------------------------
def test_peaks(mod, recset, chrom):
    for what, case, dnas in (("records", recset, recset["dnas"]), ("chromosome", chrom, [chrom["dna"]])):
        oligos, p = case["oligos"], case["p"]
        pots = case["pots"] if what == "records" else [[x] for x in case["pots"]]
        want = np.array([[peaks_from(P, per_enc, p) for P, per_enc in row] for row in pots])
        assert want.shape == (len(oligos), len(dnas), 4, 3) and (want[:, 0, :, 0] > 0).all()
        e = _engine(mod)
        got = e.scan_oligos_peaks(oligos, dnas, p)
        assert got.dtype == np.int64
        _same(got, want, f"{what}: peaks")
        tracks, got1 = e.scan_oligos_peaks(oligos, dnas, p, bin=1)
        _same(got1, want, f"{what}: peaks with tracks")
        _, ref = e.scan_oligos(oligos, dnas, p, min_value=1, track_bin=1)
        for q in range(len(oligos)):
            for r in range(len(dnas)):
                _same(tracks[q][r].array(), pots[q][r][0], f"{what}: track {q}, {r}")
                _same(tracks[q][r].array(), ref[q][r].array(), f"{what}: track {q}, {r} against scan_oligos")
                assert (tracks[q][r].units, tracks[q][r].saturated_units) == (ref[q][r].units, 0)
        nseg = sum(mod.segment_count(len(d), p) for d in dnas)
        cut = nseg // 2
        parts = [e.scan_oligos_peaks(oligos, dnas, p, seg_first=a, seg_count=c) for a, c in ((0, cut), (cut, -1))]
        e.close()
        _same(mod.merge_peaks(parts), want, f"{what}: merged shards")


# ---- 9. composition and refusals -------------------------------------------------------------------------------------------------------
def test_composition_with_the_lncrna_calls_and_refusals(mod, golden_dir, chrom):
    rna, demo = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    short = _seq(golden_dir, "h19_100")
    oligos, dna, p = chrom["oligos"], chrom["dna"], chrom["p"]
    p40 = mod.default_params(cLength=40)
    gold = open(os.path.join(golden_dir, "demo_lg40.TFOsorted"), "rb").read()
    e = _engine(mod)
    e.set_query(rna)
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold
    _check(e.scan_oligos_profile(oligos, dna, p)[0], chrom["want"][0], 24, "between two scans")
    e.scan_oligos_peaks(oligos, dna, p)
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold          # the engine's own query is still H19
    for call in (lambda: e.scan_tfo_profile(dna, p, rnas=[short], records=False), lambda: e.scan_records_track([dna], p, rnas=[short], records=False)):
        with pytest.raises(mod.FasimError) as ei:
            call()
        assert ei.value.code == mod.E_UNSUPPORTED
    cases = [(dict(oligos=[]), mod.E_ARG), (dict(oligos=[oligos[0], b""]), mod.E_ARG), (dict(oligos=[oligos[0], b"GA" * 56 + b"G"]), mod.E_ARG),
             (dict(params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED), (dict(dnas=[]), mod.E_ARG)]
    for fn in (e.scan_oligos_profile, e.scan_oligos_peaks):
        for kw, code in cases:
            kw = dict(dict(oligos=oligos, dnas=dna, params=p), **kw)
            with pytest.raises(mod.FasimError) as ei:
                fn(kw.pop("oligos"), kw.pop("dnas"), **kw)
            assert ei.value.code == code, (fn.__name__, kw, str(ei.value))
            if "113" in str(ei.value):
                assert "oligo 1" in str(ei.value)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_peaks(oligos, dna, p, bin=-1)
    assert ei.value.code == mod.E_ARG
    # the NULL outputs and the bin / out_tracks pairs, through the C interface
    L, C = mod.lib(), ctypes
    arr, lens = (C.c_char_p * 1)(oligos[0]), (C.c_int32 * 1)(len(oligos[0]))
    offs, rlens = (C.c_int64 * 1)(0), (C.c_int64 * 1)(len(dna))
    trks, pks = (C.POINTER(mod._Track) * 1)(), (mod._Peak * 4)()
    head = (e._h, arr, lens, 1, dna, offs, rlens, 1, 0, -1, C.byref(p))
    assert L.fasim_scan_oligos_profile(*head, 0, None, None) == mod.E_ARG
    assert L.fasim_scan_oligos_peaks(*head, 0, None, None, None) == mod.E_ARG
    assert L.fasim_scan_oligos_peaks(*head, 0, trks, pks, None) == mod.E_ARG
    assert L.fasim_scan_oligos_peaks(*head, 1, None, pks, None) == mod.E_ARG
    assert L.fasim_scan_oligos_peaks(*head, -1, trks, pks, None) == mod.E_ARG
    # the engine is usable afterwards
    _check(e.scan_oligos_profile(oligos, dna, p)[1], chrom["want"][1], 24, "after the refusals")
    assert mod.tfosorted(e.scan(demo, p40), "chr11", 2158478, p40) == gold
    e.close()


# ---- 10. the CLI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(mod, golden_dir, tmp_path_factory):
    """test_gpu_oligos.test_cli_panel's inputs: three oligos, the demo record, the first three MEG3 peaks as a record set; the
    Python results the CLI's files must equal."""
    wd = tmp_path_factory.mktemp("oligo_profile_cli")
    oligos = _panel(golden_dir, (20, 31, 112))
    names = ["tfo20", "tfo31", "tfo112"]
    (wd / "panel.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), o) for n, o in zip(names, oligos)))
    (wd / "testDNA.fa").write_bytes(open(os.path.join(golden_dir, "testDNA.fa"), "rb").read())
    demo = _seq(golden_dir, "testDNA")
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:3]
    (wd / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    p = mod.default_params()
    e = _engine(mod)
    one = e.scan_oligos_profile(oligos, demo, p)
    many = e.scan_oligos_profile(oligos, [s for _, s in peaks], p)
    pk = e.scan_oligos_peaks(oligos, [s for _, s in peaks], p)
    e.close()
    assert all(x.array().max() >= 40 for x in one + many) and (pk[:, :, :, 0] > 0).all()
    regions = []
    for k, (h, s) in enumerate(peaks):
        name, chro, span = h.split("|")
        start = int(span.split("-")[0]) - 1
        regions.append(mod.Region(k + 1, chro, start, start + len(s), name))
    segs = [mod.segment_count(len(s), p) for _, s in peaks]
    return dict(wd=wd, oligos=oligos, names=names, peaks=peaks, p=p,
                plain={f"hg19-{n}-testDNA-TFOprofile": mod.tfo_profile_tsv(one[q], oligos[q], n) for q, n in enumerate(names)},
                sets={f"{n}-recs.tfoprofile.tsv": mod.tfo_profile_tsv(many[q], oligos[q], n) for q, n in enumerate(names)},
                screens={f"{n}-recs.screen.tsv": mod.screen_tsv(regions, segs, pk[q]) for q, n in enumerate(names)})


def _cli(cli, out, f1, *extra):
    (cli["wd"] / out).mkdir()
    _run(cli["wd"], "-f1", f1, "-f2", "panel.fa", "-O", out + "/", "--oligos", *extra)
    return _files(cli["wd"] / out)


def test_cli_profile(cli):
    assert _cli(cli, "plain", "testDNA.fa", "--oligo-profile") == cli["plain"]
    assert _cli(cli, "plain2", "testDNA.fa", "--oligo-profile", "--devices", "0,0") == cli["plain"]
    assert _cli(cli, "all", "recs.fa", "--oligo-profile", "--all-records") == cli["sets"]
    assert _cli(cli, "all2", "recs.fa", "--oligo-profile", "--all-records", "--devices", "0,0") == cli["sets"]


def test_cli_with_sites_and_screen(cli):
    """The sites files and the panel table are byte for byte what the run writes without the two flags; the new files are the Python
    results' tables."""
    base = _cli(cli, "sites", "recs.fa", "--sites", "40", "--sites-gap", "3", "--all-records")
    assert len(base) == 4 and all(b"\n" in v for v in base.values())
    both = _cli(cli, "both", "recs.fa", "--sites", "40", "--sites-gap", "3", "--oligo-profile", "--oligo-screen", "--all-records")
    assert both == dict(base, **cli["sets"], **cli["screens"])
    both2 = _cli(cli, "both2", "recs.fa", "--sites", "40", "--sites-gap", "3", "--oligo-profile", "--oligo-screen", "--all-records", "--devices", "0,0")
    assert both2 == both


def test_cli_regions_screen(cli, mod):
    """The three records as BED intervals of a FASTA that holds them at their genome positions' offsets: one chromosome-like record
    per peak, the interval being the whole record."""
    wd, p = cli["wd"], cli["p"]
    fa, bed, regions = b"", b"", []
    for k, (h, s) in enumerate(cli["peaks"]):
        name = h.split("|")[0]
        fa += f">ctg{k}\n".encode() + b"ACGT" * 25 + s + b"TTGCA" * 20 + b"\n"
        bed += f"ctg{k}\t100\t{100 + len(s)}\t{name}\n".encode()
        regions.append(mod.Region(k + 1, f"ctg{k}", 100, 100 + len(s), name))
    (wd / "ctg.fa").write_bytes(fa)
    (wd / "iv.bed").write_bytes(bed)
    e = _engine(mod)
    pk = e.scan_oligos_peaks(cli["oligos"], [s for _, s in cli["peaks"]], p)
    e.close()
    segs = [mod.segment_count(len(s), p) for _, s in cli["peaks"]]
    want = {f"{n}-ctg.screen.tsv": mod.screen_tsv(regions, segs, pk[q]) for q, n in enumerate(cli["names"])}
    assert _cli(cli, "reg", "ctg.fa", "--oligo-screen", "--regions", "iv.bed") == want
