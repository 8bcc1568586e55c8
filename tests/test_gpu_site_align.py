"""Site hits on the GPU (fasim_scan_records_sites_aligned, k_site_ends / k_site_path, `fasim --sites V --sites-align`): exact equality
with the numpy restatement of test_site_align_cpu.py (which never calls the code under test) -- the (n, 8) array, the CIGAR strings
and every field of the triplex records, the two floats as float32 bit patterns -- over thresholds and gaps; segment edges and pad-row
echoes; the overlap of two segments under batches, workers, the f16 switch and resident DNA; gaps of both kinds; a 113-nt and a
three-tile query; real DNA; shards; refusals and the default path; the CLI.  GPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import encode_unit
from test_sites_cpu import expected_potential, sites_from
from test_site_align_cpu import hits_array, rescore, site_hits
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

SEVEN = ("segments", "segments_skipped", "units", "candidates", "align_calls", "logical_cells", "cells_stage2")
INTS = ("stari", "endi", "starj", "endj", "strand", "reverse", "rule", "nt", "seg", "enc")
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


class Case:
    """One (query, record, parameters): the restatement's potential, computed once, and its hits, computed once per peak (a hit
    is a function of the site's value, position and encoding and of the selected segments)."""

    def __init__(self, rna, dna, p):
        self.rna, self.dna, self.p = rna, dna, p
        self.P, self.per_enc = expected_potential(rna, dna, p)
        self.P.setflags(write=False)
        self.top = int(self.P.max())
        self._hits = {}

    def sites(self, v, gap=0):
        return sites_from(self.P, self.per_enc, v, gap)

    def hits(self, sites, seg_first=0, seg_count=-1):
        todo = [s for s in sites.tolist() if (s[3], s[4], s[5], seg_first, seg_count) not in self._hits]
        if todo:
            for s, h in zip(todo, site_hits(self.rna, self.dna, self.p, np.asarray(todo), seg_first, seg_count)):
                self._hits[(s[3], s[4], s[5], seg_first, seg_count)] = h
        return [self._hits[(s[3], s[4], s[5], seg_first, seg_count)] for s in sites.tolist()]


def _bits(x):
    return np.asarray([x], dtype=np.float32).view(np.uint32)[0]


def _check(got_sites, got_hits, want_sites, want_hits, what=""):
    """Exact equality of sites, (n, 8) array, CIGARs and records; floats as float32 bit patterns."""
    assert np.array_equal(got_sites.array(), want_sites), (what, "sites")
    want = hits_array(want_hits)
    got = got_hits.array()
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), want_sites[bad[0]].tolist())
    assert got_hits.cigars() == [h["cigar"] for h in want_hits], what
    assert got_hits.unaligned == 0 and len(got_hits) == len(want_hits)
    for k, (g, h) in enumerate(zip(got_hits.triplexes(), want_hits)):
        w = h["rec"]
        assert [g[f] for f in INTS] == [w[f] for f in INTS], (what, k, g, w)
        assert (g["tfo"], g["tts"]) == (w["tfo"], w["tts"]), (what, k)
        assert g["score"] == float(w["score"]), (what, k)
        assert (_bits(g["identity"]), _bits(g["tri_score"])) == (_bits(w["identity"]), _bits(w["tri_score"])), (what, k, g, w)


# ---- 1. thresholds and gaps ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    c = Case(_seq(golden_dir, "MEG3"), _chromosome_like(), mod.default_params(rule=1, strand=0))
    v60 = max(v for v in range(1, c.top + 1) if len(c.sites(v)) >= 60)
    c.vs = (c.top, int(0.8 * c.top), v60)
    return c


@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("records", [False, True])
def test_thresholds_and_gaps_equal_the_restatement(mod, chrom, gap, records):
    e = _engine(mod, chrom.rna)
    plain = e.scan_records([chrom.dna], chrom.p) if records else None
    for v in chrom.vs:
        want_sites = chrom.sites(v, gap)
        res, sites, hits = e.scan_sites_aligned(chrom.dna, chrom.p, min_value=v, max_gap=gap, records=records)
        _, only = e.scan_sites(chrom.dna, chrom.p, min_value=v, max_gap=gap, records=False)
        assert np.array_equal(sites[0].array(), only[0].array()) and sites[0].raw_runs == only[0].raw_runs
        _check(sites[0], hits[0], want_sites, chrom.hits(want_sites), f"V {v} G {gap}")
        if records:
            x, y = res[0], plain[0]
            assert (x.count, x.recs, x.pool) == (y.count, y.recs, y.pool) and [x.stats[k] for k in SEVEN] == [y.stats[k] for k in SEVEN]
        else:
            assert res is None
    assert len(chrom.sites(chrom.vs[2])) >= 60
    e.close()


# ---- planted records -------------------------------------------------------------------------------------------------------------------
def _for_enc(piece: bytes, enc: int) -> bytes:
    """DNA whose unit under `enc` reads `piece` (letters of the rule's output alphabet; U as T is not needed: GT pieces only)."""
    inv = {}
    for base, o in zip("ATGC", synth.RULE_OUT[enc]):
        inv.setdefault(o, base)
    d = "".join(inv[chr(c)] for c in piece).encode()
    return d[::-1] if enc & 1 else d


def _gt(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"GT", dtype=np.uint8), size=n).tobytes())


def _planted_case(mod):
    """Cases 2-4 and 7: a seeded 1 000-nt query (8 pad rows) x a 10 kb record (segments [0, 5 000), [4 900, 9 900), [9 800, 10 000))
    with hits that end on the last base of a full and of the short last segment, start on a segment's first base, end on the
    query's last row under an odd encoding, lie wholly inside the overlap of two segments, and carry a 2-base insertion and a
    2-base deletion."""
    rna = bytearray(np.random.default_rng(1000).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=1000).tobytes())
    a, b, c, d, g = _gt(1, 40), _gt(2, 40), _gt(3, 40), _gt(4, 40), _gt(5, 82)
    rna[100:140], rna[300:340], rna[500:540], rna[960:1000], rna[700:782] = a, b, c, d, g
    rna = bytes(rna)
    dna = bytearray(b"N" * 10000)              # rule 1 turns every base into G or T: a background of N keeps the plants apart
    dna[0:40] = _for_enc(a, 0)                       # starts on the first base of segment 0
    dna[4960:5000] = _for_enc(b, 0)                  # ends on the last base of the full segment 0 (and lies in segment 1 too)
    dna[9960:10000] = _for_enc(b, 12)                # ends on the last base of the short last segment
    dna[4905:4935] = _for_enc(c[:30], 0)             # wholly inside the overlap [4 900, 5 000) of segments 0 and 1
    dna[2000:2040] = _for_enc(d, 1)                  # the query's last rows under an odd encoding: echoed by the pad rows
    dna[7000:7040] = _for_enc(d, 13)
    dna[3000:3080] = _for_enc(g[:40] + g[42:], 0)    # two query bases against a gap: I
    dna[6000:6084] = _for_enc(g[:41], 12) + b"CC" + _for_enc(g[41:], 12)      # two target bases against a gap: D
    p = mod.default_params(rule=1, strand=0)
    case = Case(rna, bytes(dna), p)
    case.v = 100
    return case


@pytest.fixture(scope="module")
def planted(mod):
    return _planted_case(mod)


def test_edges_echoes_and_gaps(mod, planted):
    want_sites = planted.sites(planted.v)
    want = planted.hits(want_sites)
    assert any(h["jp"] - h["j1"] > 0 for h in want) and any(h["j1"] == h["n"] - 1 for h in want) and any(h["j0"] == 0 for h in want)
    assert any(h["i1"] == len(planted.rna) - 1 and h["enc"] & 1 for h in want)
    assert any("I" in h["cigar"] for h in want) and any("D" in h["cigar"] for h in want)
    assert any(h["n"] == 200 for h in want)
    e = _engine(mod, planted.rna)
    _, sites, hits = e.scan_sites_aligned(planted.dna, planted.p, min_value=planted.v, records=False)
    e.close()
    _check(sites[0], hits[0], want_sites, want, "planted")
    for s, h in zip(want_sites.tolist(), want):          # consequence (a)
        a = h["seg"] * 4900
        seg = planted.dna[a:a + 5000]
        assert rescore(planted.rna, encode_unit(seg, h["enc"]), h["i0"], h["j0"], h["cigar"]) == (s[3], h["i1"], h["j1"])


@pytest.mark.parametrize("options", [dict(seg_batch=1, workers=1), dict(seg_batch=3, workers=16), dict(workers=16), dict(dp_f16=0), dict(dp_f16=1)])
def test_overlap_takes_the_smaller_segment_whatever_the_batches(mod, planted, options):
    want_sites = planted.sites(planted.v)
    want = planted.hits(want_sites)
    inside = [h for s, h in zip(want_sites.tolist(), want) if 4905 <= s[1] and s[2] <= 4955 and s[5] == 0]
    assert inside and all(h["seg"] == 0 and h["j0"] >= 4905 and "30M" == h["cigar"] for h in inside)
    e = _engine(mod, planted.rna, **options)
    _, sites, hits = e.scan_sites_aligned([planted.dna], planted.p, min_value=planted.v, records=False)
    _check(sites[0], hits[0], want_sites, want, str(options))
    if options == dict(dp_f16=1):
        e.load_dna(planted.dna)
        _, sites, hits = e.scan_sites_aligned(None, planted.p, min_value=planted.v, records=False)
        _check(sites[0], hits[0], want_sites, want, "resident")
    e.close()


# ---- 5. small and tiled queries ------------------------------------------------------------------------------------------------------
def test_a_113_nt_query_and_three_query_tiles(mod):
    p = mod.default_params(rule=1, strand=0)
    rna = bytes(np.random.default_rng(113).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=113).tobytes())
    small = Case(rna, synth.planted_dna(5300, 21, rna, every=700, min_len=25, max_len=60), p)
    rna = bytes(np.random.default_rng(8007).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=7000).tobytes())
    tiled = Case(rna, synth.planted_dna(6000, 17, rna), p)
    for what, c in (("113 nt", small), ("7 000 nt", tiled)):
        v = int(0.8 * c.top)
        want_sites = c.sites(v)
        assert len(want_sites) >= 1
        e = _engine(mod, c.rna)
        _, sites, hits = e.scan_sites_aligned(c.dna, c.p, min_value=v, records=False)
        e.close()
        _check(sites[0], hits[0], want_sites, c.hits(want_sites), what)


def test_a_query_whose_row_state_lives_in_hbm(mod):
    """Above 8 192 rows k_site_ends keeps the row state and reads the query codes in HBM: a seeded 8 300-nt query (four pad rows)
    x the 6 kb planted record, by the same exact comparison."""
    p = mod.default_params(rule=1, strand=0)
    rna = bytes(np.random.default_rng(8300).choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=8300).tobytes())
    c = Case(rna, synth.planted_dna(6000, 17, rna), p)
    v = int(0.8 * c.top)
    want_sites = c.sites(v)
    want = c.hits(want_sites)
    assert len(want_sites) >= 2 and len({h["seg"] for h in want}) == 2 and max(h["i1"] for h in want) > 0
    e = _engine(mod, c.rna)
    _, sites, hits = e.scan_sites_aligned(c.dna, c.p, min_value=v, records=False)
    e.close()
    _check(sites[0], hits[0], want_sites, want, "8 300 nt")


# ---- 6. real DNA -----------------------------------------------------------------------------------------------------------------------
def test_first_24_peaks_equal_the_restatement(mod, golden_dir):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dnas = [s for _, s in helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:24]]
    e = _engine(mod, rna)
    _, _, pk = e.scan_records_track(dnas, p, bin=0, records=False)
    _, prof = e.scan_tfo_profile(dnas, p, per_record=True, records=False)
    _, sites, hits = e.scan_sites_aligned(dnas, p, min_value=60, records=False)
    e.close()
    nhits = 0
    for r, dna in enumerate(dnas):
        c = Case(rna, dna, p)
        want_sites = c.sites(60)
        _check(sites[r], hits[r], want_sites, c.hits(want_sites), f"record {r}")
        R = prof[r].array()
        a, h = sites[r].array(), hits[r].array()
        nhits += len(a)
        for cls in range(4):
            mine = np.flatnonzero(a[:, 0] == cls)
            assert all(R[cls][h[k, 3]] >= a[k, 3] for k in mine)                 # consequence (b)
            if len(mine):
                best = mine[np.argmax(a[mine, 3])]
                assert R[cls][h[best, 3]] == a[best, 3] and a[best, [3, 4, 5]].tolist() == pk[r, cls].tolist()
    assert nhits > 48


# ---- 7. shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [((0, 1), (1, -1)), ((0, 1), (1, 1), (2, -1))])
def test_shards_merge_to_the_whole(mod, planted, cuts):
    """The first split falls between segments 0 and 1, whose overlap holds a hit: shard 1 sees it in segment 1, the merge keeps
    segment 0's."""
    want_sites = planted.sites(planted.v)
    want = planted.hits(want_sites)
    e = _engine(mod, planted.rna)
    sp, hp = [], []
    for first, count in cuts:
        _, s, h = e.scan_sites_aligned(planted.dna, planted.p, min_value=planted.v, records=False, seg_first=first, seg_count=count)
        Pk, pk = expected_potential(planted.rna, planted.dna, planted.p, first, count)
        part_sites = sites_from(Pk, pk, planted.v)
        _check(s[0], h[0], part_sites, planted.hits(part_sites, first, count), f"shard {first} {count}")
        sp.append(s[0]); hp.append(h[0])
    e.close()
    k = [i for i, s in enumerate(sp[1].array().tolist()) if 4905 <= s[1] and s[2] <= 4955 and s[5] == 0]
    assert k and all(hp[1].array()[i, 0] == first_of_second for i in k for first_of_second in [cuts[1][0]])
    ms, mh = mod.merge_site_hits(sp, hp)
    _check(ms, mh, want_sites, want, "merged")
    assert np.array_equal(ms.array(), mod.merge_sites(sp).array())


# ---- 8. refusals and the default path ------------------------------------------------------------------------------------------------
def test_refusals_and_the_default_path(mod, golden_dir, planted):
    rna, dna, p = planted.rna, planted.dna, planted.p
    short = _seq(golden_dir, "h19_100")
    e = _engine(mod, rna)
    before = (e.scan_sites(dna, p, min_value=planted.v)[1][0].array(), e.scan_records([dna], p)[0], e.scan_track(dna, p, bin=25, records=False)[1].array())
    cases = [(dict(min_value=0), mod.E_ARG), (dict(min_value=16384), mod.E_ARG), (dict(min_value=60, max_gap=-1), mod.E_ARG),
             (dict(min_value=60, rnas=[short]), mod.E_UNSUPPORTED), (dict(min_value=60, params=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED)]
    for kw, code in cases:
        kw = dict(kw)
        kw.setdefault("params", p)
        with pytest.raises(mod.FasimError) as ei:
            e.scan_sites_aligned(dna, **kw)
        assert ei.value.code == code, (kw, str(ei.value))
    L, C = mod.lib(), __import__("ctypes")
    offs, lens = (C.c_int64 * 1)(0), (C.c_int64 * 1)(len(dna))
    sts = (C.POINTER(mod._Sites) * 1)()
    rc = L.fasim_scan_records_sites_aligned(e._h, None, None, 0, dna, offs, lens, 1, 0, -1, C.byref(p), 60, 0, None, sts, None, None)
    assert rc == mod.E_ARG
    want_sites = planted.sites(planted.v)
    res, sites, hits = e.scan_sites_aligned(dna, p, min_value=planted.v)
    _check(sites[0], hits[0], want_sites, planted.hits(want_sites), "after the refusals")
    after = (e.scan_sites(dna, p, min_value=planted.v)[1][0].array(), e.scan_records([dna], p)[0], e.scan_track(dna, p, bin=25, records=False)[1].array())
    e.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    for x in (after[1], res[0]):
        assert (x.count, x.recs, x.pool) == (before[1].count, before[1].recs, before[1].pool)


# ---- 9. the CLI ------------------------------------------------------------------------------------------------------------------------
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
    _, sites, hits = e.scan_sites_aligned(dna, p, min_value=100, records=False)
    e.close()
    assert hits[0].unaligned == 0 and len(hits[0]) > 4
    bed = mod.sites_bed(sites[0], "chr11", 2158478, "H19")
    tsv = mod.site_hits_tsv(sites[0], hits[0], "chr11", 2158478, "H19")
    lines = tsv.splitlines()
    assert lines[0] == b"# fasim site hits lncRNA=H19 min_value=100 max_gap=0" and len(lines) == 2 + len(hits[0])
    assert all(len(x.split(b"\t")) == 15 for x in lines[1:])
    for x, s in zip(lines[2:], bed.splitlines()[1:]):
        f, b = x.split(b"\t"), s.split(b"\t")
        assert (f[0], f[3], f[4], f[5]) == (b[0], b[3], b[4], b[5])
        assert int(f[1]) <= int(b[6]) < int(f[2])                       # the peak lies on a DNA base of the hit
        assert len(f[13]) == len(f[14]) == int(f[9]) and re.fullmatch(rb"(\d+[MID])+", f[12])

    def run(out, *extra, status=0):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra, status=status)
        return _files(tmp_path / out)

    name = "hg19-H19-testDNA-TFOsites-100"
    base = run("sites", "--sites", "100")
    assert base[name] == bed and len(base) == 4
    assert run("full", "--sites", "100", "--sites-align") == dict(base, **{name + "-aligned": tsv})
    assert run("two", "--sites", "100", "--sites-align", "--devices", "0,0") == dict(base, **{name + "-aligned": tsv})
    assert run("only", "--sites", "100", "--sites-only", "--sites-align") == {name: bed, name + "-aligned": tsv}
    for k, extra in enumerate((["--sites-align"], ["--sites-align", "--sites", "100", "-F"], ["--sites-align", "--sites", "100", "--track", "25"])):
        assert run(f"refused{k}", *extra, status=2) == {}, extra


def test_cli_record_sets(mod, golden_dir, tmp_path):
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:8]
    (tmp_path / "MEG3.fa").write_bytes(open(os.path.join(golden_dir, "MEG3.fa"), "rb").read())
    lnc = synth.read_fasta(str(tmp_path / "MEG3.fa"))[0]
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    e = _engine(mod, rna)
    _, sites, hits = e.scan_sites_aligned([s for _, s in peaks], p, min_value=60, records=False)
    head = (b"# fasim site hits lncRNA=%s min_value=60 max_gap=0\n" % lnc.encode() +
            b"chrom\ttts_start\ttts_end\tclass\tvalue\tstrand\trule\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tTFO\tTTS\tname\n")
    want = head
    for (h, s), st, ht in zip(peaks, sites, hits):
        name, chro, span = h.split("|")
        want += mod.site_hits_tsv(st, ht, chro, int(span.split("-")[0]), lnc, record_name=name, header=False)
    assert want.count(b"\n") > 10 and all(len(line.split(b"\t")) == 16 for line in want.splitlines()[1:])

    def run(out, f1, *extra):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", "MEG3.fa", "-O", out + "/", *extra)
        return _files(tmp_path / out)

    bed, tsv = f"{lnc}-recs.sites-60.bed", f"{lnc}-recs.sites-60.aligned.tsv"
    base = run("all", "recs.fa", "--all-records", "--sites", "60", "--sites-only")
    assert run("alla", "recs.fa", "--all-records", "--sites", "60", "--sites-only", "--sites-align") == dict(base, **{tsv: want})
    assert list(base) == [bed]
    # --regions: overlapping and repeated intervals of one chromosome
    g = b"".join(s for _, s in peaks[:4])
    (tmp_path / "g.bed").write_text(f"chrA\t1000\t5900\tlen4900\nchrA\t3000\t9000\nchrA\t3500\t4200\tinner\nchrA\t{len(g) - 3000}\t{len(g)}\ttail\n")
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + g + b"\n")
    regs = mod.read_bed(tmp_path / "g.bed")
    _, sites, hits = e.scan_sites_aligned([g[r.start:r.end] for r in regs], p, min_value=60, max_gap=5, records=False)
    e.close()
    want = head.replace(b"max_gap=0", b"max_gap=5")
    for r, st, ht in zip(regs, sites, hits):
        want += mod.site_hits_tsv(st, ht, r.chrom, r.start + 1, lnc, record_name=r.name, header=False)
    tsv = f"{lnc}-genome.sites-60.aligned.tsv"
    args = ("genome.fa", "--regions", "g.bed", "--sites", "60", "--sites-gap", "5", "--sites-only")
    base = run("reg", *args)
    assert run("rega", *args, "--sites-align") == dict(base, **{tsv: want})
    assert run("rega2", *args, "--sites-align", "--devices", "0,0") == dict(base, **{tsv: want})


# ---- an untidy query ----------------------------------------------------------------------------------------------------------------
def test_untidy_query(mod):
    """helpers.dirty_case(700) (U, lower case, N R Y n u in the query) under rule 8: k_site_ends and k_site_path read the query as
    stage 3 does (U as A, every other letter -4), and the records show the query's letters as they were written, which the
    identity counts as mismatches and the stability scores 0.  Hits over each class of untidy row."""
    rna, dna = helpers.dirty_case(700)
    c = Case(rna, dna, mod.default_params(rule=8, strand=0))
    assert c.top >= 150
    rows = helpers.dirty_rows(rna)
    e = _engine(mod, rna)
    for v in (c.top, int(0.8 * c.top)):
        want_sites = c.sites(v)
        want_hits = c.hits(want_sites)
        _, sites, hits = e.scan_sites_aligned(dna, c.p, min_value=v, records=False)
        _check(sites[0], hits[0], want_sites, want_hits, f"V {v}")
    over = {k: sum(any(h["rec"]["stari"] - 1 <= r <= h["rec"]["endi"] - 1 for r in rr) for h in want_hits) for k, rr in rows.items()}
    print("hits over untidy rows at 0.8 of the top:", over)
    assert min(over.values()) >= 5
    e.close()
