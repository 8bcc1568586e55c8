"""The hits of oligo sites on the GPU (fasim_scan_oligos_aligned, k_site_ends_short + k_site_path, `fasim --oligos --sites V
--oligo-hits`): exact equality with the numpy restatement of section 15 (test_site_align_cpu.py::site_hits, which never calls the
code under test) -- the (n, 8) array, the CIGAR strings, every field of the records, the two floats as float32 bit patterns -- over
the length edges 1 .. 112 nt (every ROWS build of the kernel, both sides of each multiple of 16) and the segment edges; the switch
site_short; batches, workers, shards, resident DNA, panel order, composition with the lncRNA call; more problems than one
workgroup and one chunk; the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import encode_unit
from test_site_align_cpu import hits_array, rescore
from test_gpu_site_align import Case, _check
from test_gpu_oligos import _pre_image

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")
LENGTHS = (1, 15, 16, 17, 20, 29, 32, 33, 48, 64, 80, 96, 100, 112)
N = 5100                  # two segments: [0, 5 000) and [4 900, 5 100), the second 200 nt


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _engine(mod, rna=None, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    if rna is not None:
        e.set_query(rna)
    return e


def _gt(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"GT", dtype=np.uint8), size=n).tobytes())


def _oligo(m):
    """An oligo over G and T, which rule 1 pairs in full."""
    return _gt(1800 + m, m)


def threshold(m):
    """A value that every plant of _records reaches: the better half of the oligo."""
    return max(5, 5 * (m - m // 2))


def _records(oligo):
    """Two records of 5 100 nt over a background of N (rule 1 turns every base into G or T: N keeps the plants apart) with a
    300-nt random stretch.  Plants of the oligo, as pre-images under the four encodings of rule 1: exact at offset 0 (record a)
    and 3 (record b); mismatched; with the largest DNA-side gap that the two halves still pay for; with two oligo bases missing;
    across the end of segment 0 under a mirrored encoding (record a: its peak lies in the overlap, segment 0 holds half of it:
    a problem of level 1); exact at n - m (record b)."""
    m = len(oligo)
    rng = np.random.default_rng(1900 + m)
    h = m // 2
    d = (5 * h - 13) // 4
    out = []
    for k in (0, 1):
        dna = bytearray(b"N" * N)
        dna[2000:2300] = synth.random_dna(300, 1900 + 2 * m + k)

        def put(at, tract, enc):
            x = _pre_image(tract, enc, rng)
            dna[at:at + len(x)] = x

        put(3 * k, oligo, k)
        if m >= 2:
            flip = bytes([oligo[h] ^ (ord("G") ^ ord("T"))])
            put(400, oligo[:h] + flip + oligo[h + 1:], 1 - k)
        if d >= 1:
            put(800, oligo[:h] + b"C" * d + oligo[h:], 12 + k)      # (C has no pre-image under rule 1: random bases, then G or T)
        if m >= 15:
            put(1400, oligo[:h] + oligo[h + 2:], 13 - k)
        if k == 0:
            put(5000 - h, oligo, 1)
        else:
            put(N - m, oligo, 0)
        out.append(bytes(dna))
    return out


class Panel:
    """The yardstick of the length sweep, computed once per oligo and shared by the tests."""

    def __init__(self, p):
        self.p = p
        self._cases = {}

    def cases(self, m):
        if m not in self._cases:
            o = _oligo(m)
            self._cases[m] = [Case(o, dna, self.p) for dna in _records(o)]
        return self._cases[m]

    def want(self, m, v=None, gap=0):
        v = v or threshold(m)
        out = []
        for c in self.cases(m):
            s = c.sites(v, gap)
            out.append((s, c.hits(s)))
        return out


@pytest.fixture(scope="module")
def panel(mod):
    return Panel(mod.default_params(rule=1, strand=0))


def _same_hits(a, b, what):
    assert np.array_equal(a.array(), b.array()), what
    assert a.cigars() == b.cigars() and a.triplexes() == b.triplexes() and a.unaligned == b.unaligned, what


# ---- 1. length edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LENGTHS)
def test_length_edges_equal_the_restatement(mod, panel, m):
    o = _oligo(m)
    cases = panel.cases(m)
    v = threshold(m)
    e = _engine(mod)
    sites, hits = e.scan_oligos_aligned([o], [c.dna for c in cases], panel.p, min_value=v)
    only = e.scan_oligos([o], [c.dna for c in cases], panel.p, min_value=v)
    e.close()
    assert len(sites) == len(hits) == 1 and len(sites[0]) == len(hits[0]) == 2
    levels = gaps = 0
    for r, (c, (want_sites, want)) in enumerate(zip(cases, panel.want(m))):
        assert mod.segment_count(len(c.dna), panel.p) == 2 and c.top == 5 * m
        assert np.array_equal(sites[0][r].array(), only[0][r].array()) and sites[0][r].raw_runs == only[0][r].raw_runs
        _check(sites[0][r], hits[0][r], want_sites, want, f"{m} nt, record {r}")
        assert len(want) >= (3 if m >= 15 else 2)
        for s, h in zip(want_sites.tolist(), want):
            a = h["seg"] * 4900
            assert rescore(o, encode_unit(c.dna[a:a + 5000], h["enc"]), h["i0"], h["j0"], h["cigar"]) == (s[3], h["i1"], h["j1"])
        levels += sum(h["seg"] == 1 and s[4] < 5000 for s, h in zip(want_sites.tolist(), want))
        gaps += sum("D" in h["cigar"] for h in want) + 100 * sum("I" in h["cigar"] for h in want)
        if r == 0:
            assert any(h["j0"] == 0 or h["j1"] == h["n"] - 1 for h in want)        # the plant at offset 0
        else:
            assert any(s[2] == N for s in want_sites.tolist())                       # the plant at n - m
    if m > 1:
        assert levels >= 1, "no site whose first covering segment does not hold its value"
    if m >= 15:
        assert gaps % 100 >= 1 and gaps >= 100


# ---- 2. segment edges --------------------------------------------------------------------------------------------------------------
def test_segment_edges(mod, panel):
    """Records of 1, 7, 17, 4 999, 5 000 and 5 001 nt (the tails of one planted record), one with exactly one site (a single
    problem: the launch's only lane) and some with none, in one call with a 20-nt oligo."""
    o = _oligo(20)
    p = panel.p
    full = _records(o)[1][N - 5001:]
    dnas = [full[5001 - n:] for n in (1, 7, 17, 4999, 5000, 5001)]
    one = bytearray(b"N" * 300)
    one[100:120] = _pre_image(o, 0, np.random.default_rng(7))
    dnas += [bytes(one), b"N" * 200 + b"A"]
    v = 70
    e = _engine(mod)
    sites, hits = e.scan_oligos_aligned([o], dnas, p, min_value=v)
    e.close()
    counts = []
    for r, dna in enumerate(dnas):
        c = Case(o, dna, p)
        want_sites = c.sites(v)
        _check(sites[0][r], hits[0][r], want_sites, c.hits(want_sites), f"record {r} of {len(dna)} nt")
        counts.append(len(want_sites))
    assert counts[:3] == [0, 0, 1] and min(counts[3:6]) >= 3 and counts[6:] == [1, 0]
    assert len(hits[0][7]) == 0 and hits[0][7].array().shape == (0, 8) and hits[0][7].cigars() == []


# ---- 3. the switch -----------------------------------------------------------------------------------------------------------------
def test_site_short_switch_gives_identical_hits(mod, panel):
    """Option site_short (FASIM_SITE_SHORT) 0 runs the same problems on k_site_ends: the same arrays, CIGARs and records, on the
    panel of the length sweep in one call, at a threshold low enough for every oligo of 15 nt and more."""
    oligos = [_oligo(m) for m in LENGTHS]
    dnas = _records(_oligo(112)) + _records(_oligo(20))
    got = []
    for short in (1, 0):
        e = _engine(mod, site_short=short)
        got.append(e.scan_oligos_aligned(oligos, dnas, panel.p, min_value=40, max_gap=1))
        e.close()
    total = 0
    for q in range(len(oligos)):
        for r in range(len(dnas)):
            assert np.array_equal(got[0][0][q][r].array(), got[1][0][q][r].array())
            _same_hits(got[0][1][q][r], got[1][1][q][r], (LENGTHS[q], r))
            assert got[0][1][q][r].unaligned == 0
            total += len(got[0][1][q][r])
    assert total >= 40


# ---- 4. batches, workers, shards, resident DNA, panel order, composition -----------------------------------------------------------
def test_engine_paths(mod, panel, golden_dir):
    ms = (20, 33, 112)
    oligos = [_oligo(m) for m in ms]
    dnas = [c.dna for c in panel.cases(112)]
    v = 50
    rna = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    p40 = mod.default_params(cLength=40)
    e = _engine(mod, rna)
    _, s0, h0 = e.scan_sites_aligned(demo, p40, min_value=100, records=False)
    sites, hits = e.scan_oligos_aligned(oligos, dnas, panel.p, min_value=v)
    # the 112-nt oligo against its own records: the yardstick
    for r, c in enumerate(panel.cases(112)):
        want_sites = c.sites(v)
        _check(sites[2][r], hits[2][r], want_sites, c.hits(want_sites), f"record {r}")
    assert sum(len(h) for row in hits for h in row) >= 12
    # the engine's own lncRNA is neither read nor changed
    _, s1, h1 = e.scan_sites_aligned(demo, p40, min_value=100, records=False)
    assert np.array_equal(s0[0].array(), s1[0].array()) and len(h0[0]) > 4
    _same_hits(h0[0], h1[0], "the lncRNA call after the panel")
    # shards of the segment list (2 + 2 segments), merged
    parts = [e.scan_oligos_aligned(oligos, dnas, panel.p, min_value=v, seg_first=a, seg_count=c) for a, c in ((0, 1), (1, -1))]
    for q in range(3):
        for r in range(2):
            ms_, mh = mod.merge_site_hits([x[0][q][r] for x in parts], [x[1][q][r] for x in parts])
            assert np.array_equal(ms_.array(), sites[q][r].array())
            _same_hits(mh, hits[q][r], ("merged shards", q, r))
    # resident DNA equals the streamed record
    e.load_dna(dnas[0])
    rs, rh = e.scan_oligos_aligned(oligos, None, panel.p, min_value=v)
    for q in range(3):
        assert np.array_equal(rs[q][0].array(), sites[q][0].array())
        _same_hits(rh[q][0], hits[q][0], ("resident", q))
    # a permuted panel gives permuted results
    bs, bh = e.scan_oligos_aligned(oligos[::-1], dnas, panel.p, min_value=v)
    for q in range(3):
        for r in range(2):
            assert np.array_equal(bs[2 - q][r].array(), sites[q][r].array())
            _same_hits(bh[2 - q][r], hits[q][r], ("reversed panel", q, r))
    # an oligo above 112 nt, and the outputs the call needs
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_aligned([oligos[0], b"GT" * 56 + b"G"], dnas, panel.p, min_value=v)
    assert ei.value.code == mod.E_ARG and "113" in str(ei.value)
    L, C = mod.lib(), __import__("ctypes")
    arr, lens = (C.c_char_p * 1)(oligos[0]), (C.c_int32 * 1)(len(oligos[0]))
    offs, rlens = (C.c_int64 * 1)(0), (C.c_int64 * 1)(len(dnas[0]))
    sts = (C.POINTER(mod._Sites) * 1)()
    assert L.fasim_scan_oligos_aligned(e._h, arr, lens, 1, dnas[0], offs, rlens, 1, 0, -1, C.byref(panel.p), v, 0, sts, None, None) == mod.E_ARG
    assert L.fasim_scan_oligos_aligned(e._h, arr, lens, 1, dnas[0], offs, rlens, 1, 0, -1, C.byref(panel.p), v, 0, None, None, None) == mod.E_ARG
    again = e.scan_oligos_aligned(oligos, dnas, panel.p, min_value=v)
    _same_hits(again[1][2][1], hits[2][1], "after the refusals")
    e.close()
    for options in (dict(seg_batch=1, workers=1), dict(workers=16)):
        e = _engine(mod, **options)
        os_, oh = e.scan_oligos_aligned(oligos, dnas, panel.p, min_value=v)
        e.close()
        for q in range(3):
            for r in range(2):
                assert np.array_equal(os_[q][r].array(), sites[q][r].array())
                _same_hits(oh[q][r], hits[q][r], (options, q, r))


# ---- 5. more problems than one workgroup and one chunk -----------------------------------------------------------------------------
def test_many_sites_in_several_chunks(mod):
    """A 20-nt oligo against 5 100 nt of random DNA at the value that cuts its potential into the most runs: more than 512 sites (three workgroups of k_site_ends_short and
    a partly filled last one).  Chunks of 200 problems (option site_chunk) cut the problems of a unit apart.  A sample of 200 sites
    against the yardstick, all of them against site_short = 0 and against the single chunk."""
    o = _oligo(20)
    p = mod.default_params(rule=1, strand=0)
    dna = synth.random_dna(N, 1905)
    v = 47
    got = {}
    for key, options in (("chunks", dict(site_chunk=200)), ("one", dict()), ("long", dict(site_short=0))):
        e = _engine(mod, **options)
        got[key] = e.scan_oligos_aligned([o], dna, p, min_value=v)
        e.close()
    sites, hits = got["chunks"][0][0][0], got["chunks"][1][0][0]
    assert len(hits) > 512 and hits.unaligned == 0
    for key in ("one", "long"):
        assert np.array_equal(got[key][0][0][0].array(), sites.array())
        _same_hits(got[key][1][0][0], hits, key)
    c = Case(o, dna, p)
    want_sites = c.sites(v)
    assert np.array_equal(sites.array(), want_sites)
    pick = np.sort(np.random.default_rng(1906).choice(len(want_sites), size=200, replace=False))
    want = c.hits(want_sites[pick])
    assert np.array_equal(hits.array()[pick], hits_array(want))
    cig, rec = hits.cigars(), hits.triplexes()
    for k, h in zip(pick.tolist(), want):
        assert cig[k] == h["cigar"] and (rec[k]["tfo"], rec[k]["tts"], rec[k]["nt"]) == (h["rec"]["tfo"], h["rec"]["tts"], h["rec"]["nt"])


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------------
def _run(wd, *args, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def test_cli_oligo_hits(mod, golden_dir, tmp_path):
    h19 = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    oligos = [h19[300 + 131 * k:300 + 131 * k + m] for k, m in enumerate((20, 31, 112))]
    names = ["tfo20", "tfo31", "tfo112"]
    (tmp_path / "panel.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), o) for n, o in zip(names, oligos)))
    (tmp_path / "testDNA.fa").write_bytes(open(os.path.join(golden_dir, "testDNA.fa"), "rb").read())
    demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:3]
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + s + b"\n" for h, s in peaks))
    g = b"".join(s for _, s in peaks)
    assert len(g) > 6000
    (tmp_path / "g.bed").write_text(f"chrA\t1000\t5900\tlen4900\nchrA\t500\t{len(g) - 100}\nchrA\t{len(g) - 3000}\t{len(g)}\ttail\n")
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + g + b"\n")
    regs = mod.read_bed(tmp_path / "g.bed")
    p = mod.default_params()
    e = _engine(mod)
    one = e.scan_oligos_aligned(oligos, demo, p, min_value=40, max_gap=3)
    many = e.scan_oligos_aligned(oligos, [s for _, s in peaks], p, min_value=40, max_gap=3)
    reg = e.scan_oligos_aligned(oligos, [g[r.start:r.end] for r in regs], p, min_value=40, max_gap=3)
    e.close()
    assert sum(len(h[0]) for h in one[1]) >= 3 and all(h.unaligned == 0 for row in one[1] + many[1] + reg[1] for h in row)
    plain, sets, rset = {}, {}, {}
    for q, n in enumerate(names):
        plain[f"hg19-{n}-testDNA-TFOsites-40-aligned"] = mod.site_hits_tsv(one[0][q][0], one[1][q][0], "chr11", 2158478, n)
        head = (b"# fasim site hits lncRNA=%s min_value=40 max_gap=3\n" % n.encode() +
                b"chrom\ttts_start\ttts_end\tclass\tvalue\tstrand\trule\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tTFO\tTTS\tname\n")
        text = head
        for (h, _), st, ht in zip(peaks, many[0][q], many[1][q]):
            name, chro, span = h.split("|")
            text += mod.site_hits_tsv(st, ht, chro, int(span.split("-")[0]), n, record_name=name, header=False)
        sets[f"{n}-recs.sites-40.aligned.tsv"] = text
        text = head
        for r, st, ht in zip(regs, reg[0][q], reg[1][q]):
            text += mod.site_hits_tsv(st, ht, r.chrom, r.start + 1, n, record_name=r.name, header=False)
        rset[f"{n}-genome.sites-40.aligned.tsv"] = text
    assert sum(t.count(b"\n") for t in plain.values()) >= 9

    def run(out, f1, *extra):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", "panel.fa", "-O", out + "/", "--oligos", "--sites", "40", "--sites-gap", "3", *extra)
        return _files(tmp_path / out)

    base = run("plain", "testDNA.fa")
    assert len(base) == 4 and not any(n.endswith("-aligned") for n in base)
    assert run("plainh", "testDNA.fa", "--oligo-hits") == dict(base, **plain)
    assert run("plainh2", "testDNA.fa", "--oligo-hits", "--devices", "0,0") == dict(base, **plain)
    base = run("all", "recs.fa", "--all-records")
    assert run("allh", "recs.fa", "--all-records", "--oligo-hits") == dict(base, **sets)
    assert run("allh2", "recs.fa", "--all-records", "--oligo-hits", "--devices", "0,0") == dict(base, **sets)
    base = run("reg", "genome.fa", "--regions", "g.bed")
    assert run("regh", "genome.fa", "--regions", "g.bed", "--oligo-hits", "--upper") == dict(base, **rset)
