"""The alignment behind every variant score, on the GPU (fasim_score_variants_aligned, k_touch_path, `fasim --variants
--variant-hits`): exact equality of every hit -- encoding, cells, CIGAR, nt, TFO and TTS strings -- with the restatement of
test_variant_hits_cpu.py (which never calls the code under test) over the query lengths at which the kernel takes another path, both
sides of the LDS / HBM row state, the longest query, the cell limit, all encodings and flanks, a hit that ends in a gap, independence
of the other variants and the launches, the projection of insertions and deletions to the reference, and the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import enabled_encodings, encode_unit
from test_gpu_variants import EXE, LDS_ROWS, _end_cases, _h19, _other, _query, _records, _variants
from test_variant_hits_cpu import expected_hits, span_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    return mod.Engine(0)


def _rows(hits):
    """Per hit (enc, i0, i1, j0, j1, nt, cigar_len, cigar, tfo, tts, stari, endi, starj, endj)."""
    arr, cig, tri = hits.array(), hits.cigars(), hits.triplexes()
    return [tuple(int(x) for x in arr[k, 1:]) + (cig[k], tri[k]["tfo"], tri[k]["tts"], tri[k]["stari"], tri[k]["endi"], tri[k]["starj"],
                                                tri[k]["endj"]) for k in range(hits.n)]


def _check(mod, eng, query, dnas, variants, flank, p, what):
    """One query: scores, windows and every slot's hit against the restatement; returns (call's results, the restatement's slots)."""
    got = eng.score_variants_aligned(variants, dnas, p, flank=flank, queries=[query])
    values, encs, flags, wins, hits = got
    plain = eng.score_variants(variants, dnas, p, flank=flank, queries=[query])
    for a, b in zip(got[:3], plain):
        assert np.array_equal(a, b), what
    (ev, ee, ef), ewins, slots = expected_hits(query, dnas, variants, flank, p)
    assert np.array_equal(values[0], ev) and np.array_equal(encs[0], ee) and np.array_equal(flags[0], ef), what
    assert np.array_equal(wins, ewins), (what, wins.tolist(), ewins.tolist())
    h = hits[0]
    assert h.n == 8 * len(variants) and h.unaligned == 0, (what, h.n, h.unaligned)
    arr, rows = h.array(), _rows(h)
    for v in range(len(variants)):
        for al in range(2):
            for c in range(4):
                k = mod.variant_hit_index(v, al, c)
                s = slots.get((v, al, c))
                assert arr[k, 0] == v
                if s is None:
                    assert values[0, v, al, c] == 0 and rows[k][1:10] == (-1, -1, -1, -1, 0, 0, "", "", ""), (what, v, al, c, rows[k])
                    continue
                r = s["rec"]
                want = (s["enc"], s["i0"], s["i1"], s["j0"], s["j1"], r["nt"], len([x for x in s["cigar"] if x in "MID"]), s["cigar"],
                        r["tfo"], r["tts"], r["stari"], r["endi"], r["starj"], r["endj"])
                assert rows[k] == want, (what, v, al, c, rows[k], want)
                assert mod.variant_hit_clipped(variants[v], wins[v], al, s["enc"], s["j0"], s["j1"]) == s["clipped"], (what, v, al, c)
    return got, slots


@pytest.mark.parametrize("m", [1, 20, 64, 65, 128, 129, 256, 257, 700])
def test_query_lengths_equal_the_restatement(mod, eng, golden_dir, m):
    p = mod.default_params(rule=1)
    query = _query(golden_dir, m)
    dnas = _records(query, p, 100 + m)
    _, slots = _check(mod, eng, query, dnas, _variants(mod, dnas), 300, p, f"m={m}")
    assert len(slots) >= 8


def test_h19_equals_the_restatement(mod, eng, golden_dir):
    p = mod.default_params(rule=1)
    query = _h19(golden_dir)
    dnas = _records(query, p, 7)
    _, slots = _check(mod, eng, query, dnas, _variants(mod, dnas)[:5], 300, p, "H19")
    assert any("I" in s["cigar"] or "D" in s["cigar"] for s in slots.values())      # the planted sites carry a DNA-side insertion


@pytest.mark.parametrize("m", [LDS_ROWS, LDS_ROWS + 1])
def test_both_sides_of_the_lds_boundary(mod, eng, golden_dir, m):
    p = mod.default_params(rule=1, strand=1)
    assert enabled_encodings(p) == [0, 1]
    query = _query(golden_dir, m)
    dnas = _records(query, p, 11)
    _check(mod, eng, query, dnas, _variants(mod, dnas)[:2], 300, p, f"m={m}")


def test_longest_query(mod, eng, golden_dir):
    """FASIM_MAX_QUERY rows, one SNV, flank 50: n = 101, 9.3 M cells."""
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, mod.MAX_QUERY)
    dnas = _records(query, p, 13)
    _, slots = _check(mod, eng, query, dnas, _variants(mod, dnas)[:1], 50, p, "m=MAX_QUERY")
    assert slots and all(s["n"] == 101 for s in slots.values())


def test_above_the_cell_limit_hits_are_unaligned_and_the_engine_stays_usable(mod, golden_dir):
    """m * n = 92 256 * 801 > 2^26: no path is traced; the scores are those of score_variants."""
    e = mod.Engine(0)
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, mod.MAX_QUERY)
    dnas = _records(query, p, 13)
    variants = _variants(mod, dnas)[:1]
    assert mod.MAX_QUERY * 801 > 1 << 26
    values, encs, flags, wins, hits = e.score_variants_aligned(variants, dnas, p, flank=400, queries=[query])
    plain = e.score_variants(variants, dnas, p, flank=400, queries=[query])
    assert np.array_equal(values, plain[0]) and np.array_equal(encs, plain[1]) and np.array_equal(flags, plain[2])
    assert wins.tolist() == [[400, 400, 3]]
    arr = hits[0].array()
    want = np.where(values[0].reshape(-1) > 0, -1, 0)
    assert (want == -1).any()
    assert arr[:, 7].tolist() == want.tolist() and hits[0].unaligned == int((want == -1).sum())
    small = _query(golden_dir, 40)
    dnas = _records(small, p, 14)
    _check(mod, e, small, dnas, _variants(mod, dnas)[:2], 100, p, "after the limit")
    e.close()


@pytest.mark.parametrize("flank", [0, 10, 2048])
def test_all_48_encodings_and_the_flanks(mod, eng, golden_dir, flank):
    p = mod.default_params()
    assert len(enabled_encodings(p)) == 48
    query = _query(golden_dir, 40)
    dnas = _records(query, p, 21)
    _, slots = _check(mod, eng, query, dnas, _variants(mod, dnas), flank, p, f"flank={flank}")
    clipped = [s["clipped"] for s in slots.values()]
    if flank == 0:
        assert all(s["clipped"] for (v, _, _), s in slots.items() if v < 4)
    if flank == 10:
        assert any(clipped) and not all(clipped)
    if flank == 2048:
        assert not any(s["clipped"] for (v, _, _), s in slots.items() if v in (0, 1, 2, 3, 8))


@pytest.mark.parametrize("flank", [0, 10])
def test_windows_with_an_empty_side(mod, eng, golden_dir, flank):
    """The variants on the record's first and last letters (test_gpu_variants): hits over windows of one or two pieces."""
    query, rec, variants, p = _end_cases(mod, golden_dir)
    _, slots = _check(mod, eng, query, [rec], variants, flank, p, f"ends, flank={flank}")
    assert {v for (v, _, _) in slots} == set(range(len(variants)))


def test_a_hit_that_reaches_the_allele_only_through_a_gap_ends_in_d(mod, eng):
    q = b"TGGTTGTGGTGTTGGTGGTT"
    pre = q.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A")
    assert encode_unit(pre, 0) == q
    dna = b"N" * 50 + pre + b"G" + b"N" * 50                 # (G and T read as G under encoding 0: no pair with the oligo's last T)
    p = mod.default_params(rule=1, strand=1)
    variants = [mod.Variant(1, "c", 70, "snv", "G", "T")]
    (values, encs, flags, wins, hits), slots = _check(mod, eng, q, [dna], variants, 40, p, "20M1D")
    assert values[0, 0, :, 0].tolist() == [84, 84] and encs[0, 0, :, 0].tolist() == [0, 0]
    for al in range(2):
        k = mod.variant_hit_index(0, al, 0)
        assert hits[0].cigars()[k] == "20M1D"
        assert hits[0].array()[k, 2:6].tolist() == [0, 19, 20, 40]
        assert mod.variant_hit_span(variants[0], wins[0], al, 0, 20, 40) == (50, 71)


def test_independent_of_the_other_variants_their_order_and_the_launches(mod, golden_dir):
    e = mod.Engine(0)
    p = mod.default_params()
    query = _query(golden_dir, 60)
    dnas = _records(query, p, 51)
    variants = _variants(mod, dnas)
    n = len(variants)
    base = e.score_variants_aligned(variants, dnas, p, flank=150, queries=[query])
    rows = _rows(base[4][0])
    assert sum(r[6] > 0 for r in rows) >= 16
    rev = e.score_variants_aligned(variants[::-1], dnas, p, flank=150, queries=[query])
    dup = e.score_variants_aligned(variants + variants, dnas, p, flank=150, queries=[query])
    rrev, rdup = _rows(rev[4][0]), _rows(dup[4][0])
    for v in range(n):
        mine = rows[8 * v:8 * v + 8]
        assert rrev[8 * (n - 1 - v):8 * (n - v)] == mine and rdup[8 * v:8 * v + 8] == mine and rdup[8 * (n + v):8 * (n + v) + 8] == mine
        assert np.array_equal(rev[0][0, n - 1 - v], base[0][0, v]) and np.array_equal(dup[3][n + v], base[3][v])
        one = e.score_variants_aligned([variants[v]], dnas, p, flank=150, queries=[query])
        assert _rows(one[4][0]) == mine and np.array_equal(one[0][0, 0], base[0][0, v])
    # the resident record, two queries
    queries = [_query(golden_dir, 33), _query(golden_dir, 300)]
    rec0 = [v for v in variants if v.rec == 0]
    streamed = e.score_variants_aligned(rec0, [dnas[0]], p, flank=100, queries=queries)
    e.load_dna(dnas[0])
    resident = e.score_variants_aligned(rec0, None, p, flank=100, queries=queries)
    for a, b in zip(streamed[:4], resident[:4]):
        assert np.array_equal(a, b)
    for q in range(2):
        assert _rows(streamed[4][q]) == _rows(resident[4][q])
        assert streamed[4][q].unaligned == 0
    assert _rows(streamed[4][0]) != _rows(streamed[4][1])
    e.close()


def _table(text: bytes):
    lines = text.decode().split("\n")
    assert lines[0].startswith("# fasim variant hits lncRNA=") and lines[-1] == ""
    names = lines[1].split("\t")
    return [dict(zip(names, x.split("\t"))) for x in lines[2:-1]]


def test_insertion_and_deletion_project_to_the_reference(mod, eng, golden_dir):
    p = mod.default_params()
    query = _query(golden_dir, 60)
    dnas = _records(query, p, 61)
    d = dnas[0]
    # an insertion and a deletion in the middle of the planted sites, so that hits run across the alleles
    variants = [mod.Variant(1, "c", 1000, "ins", d[1000:1001].decode(), d[1000:1001].decode() + "GAGA"),
                mod.Variant(2, "c", 1200, "del", d[1200:1206].decode(), d[1200:1201].decode()),
                mod.Variant(3, "c", 1005, "ins2", d[1005:1006].decode(), d[1005:1006].decode() + "TTTTTTTT"),
                mod.Variant(4, "c", 995, "del2", d[995:1001].decode(), d[995:996].decode())]
    (values, encs, flags, wins, hits), slots = _check(mod, eng, query, dnas, variants, 120, p, "indels")
    rows = _table(mod.variant_hits_tsv(variants, values[0], encs[0], wins, hits[0], 120, "Q"))
    order = [(v, al, c) for v in range(4) for al in range(2) for c in range(4) if (v, al, c) in slots]
    assert len(rows) == len(order)
    kinds = set()
    for row, (v, al, c) in zip(rows, order):
        s, x = slots[(v, al, c)], variants[v]
        alen = len(x.alt) if al else len(x.ref)
        pre, post = int(wins[v][0]), int(wins[v][1])
        start, end = span_ref(x.pos, len(x.ref), alen, pre, post, s["enc"], s["j0"], s["j1"])
        assert (int(row["tts_start"]), int(row["tts_end"])) == (start, end), (row, s)
        assert (row["id"], row["allele"], row["class"], int(row["value"])) == (x.id, "alt" if al else "ref", mod.TRACK_CLASSES[c], int(values[0, v, al, c]))
        assert (row["cigar"], row["TFO"], row["TTS"], int(row["tfo_start"]), int(row["tfo_end"]), int(row["nt"]), int(row["clipped"])) == \
            (s["cigar"], s["rec"]["tfo"], s["rec"]["tts"], s["i0"] + 1, s["i1"] + 1, s["rec"]["nt"], int(s["clipped"]))
        n = s["n"]
        w0, w1 = (n - 1 - s["j1"], n - 1 - s["j0"]) if s["enc"] & 1 else (s["j0"], s["j1"])
        if al and w0 < pre and w1 >= pre + alen:
            kinds.add("across")
            assert end - start == (w1 - w0 + 1) + len(x.ref) - alen
    assert "across" in kinds


def test_cli_writes_the_hits_table_beside_an_unchanged_variants_table(mod, eng, tmp_path, golden_dir):
    q = _query(golden_dir, 60)
    p = mod.default_params()
    dnas = _records(q, p, 41)
    chr1, chr2 = dnas
    synth.write_fasta(str(tmp_path / "g.fa"), "chr1 test record", chr1)
    with open(tmp_path / "g.fa", "a") as f:
        f.write(">chr2\n" + chr2.decode() + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + q.decode() + "\n")

    def ref(d, pos1, n=1):
        return d[pos1 - 1:pos1 - 1 + n].decode()
    good = [f"chr1\t1001\trs1\t{ref(chr1, 1001)}\t{_other(chr1[1000:1001])}\n",
            f"chr1\t1201\trs2\t{ref(chr1, 1201, 2)}\t{ref(chr1, 1201)},{ref(chr1, 1201, 2)}GG\n",
            f"chr2\t251\trs3\t{ref(chr2, 251)}\t{_other(chr2[250:251])}\n"]
    lost = "chr7\t10\tlost\tA\tC\n"
    for name, text, status in (("good.vcf", "".join(good), 0), ("all.vcf", good[0] + lost + good[1] + good[2], 1)):
        (tmp_path / name).write_text(text)
        outs = {}
        for flag in ((), ("--variant-hits",)):
            out = tmp_path / ("out_" + name + ("_hits" if flag else ""))
            out.mkdir()
            r = subprocess.run([EXE, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--variants", name, "--variant-flank", "150", *flag],
                               cwd=tmp_path, capture_output=True, text=True, timeout=120)
            assert r.returncode == status, r.stderr
            outs[bool(flag)] = out
        assert sorted(os.listdir(outs[False])) == ["Q-g.variants.tsv"]
        assert sorted(os.listdir(outs[True])) == ["Q-g.variants.hits.tsv", "Q-g.variants.tsv"]
        assert (outs[True] / "Q-g.variants.tsv").read_bytes() == (outs[False] / "Q-g.variants.tsv").read_bytes()
        variants = [v._replace(rec=1 if v.chrom == "chr2" else 0) for v in mod.read_vcf(str(tmp_path / name))]
        matched = [v.id.startswith("rs") for v in variants]
        score = [v if ok else v._replace(usable=False) for v, ok in zip(variants, matched)]
        values, encs, flags, wins, hits = eng.score_variants_aligned(score, dnas, p, flank=150, queries=[q])
        want = mod.variant_hits_tsv(variants, values[0], encs[0], wins, hits[0], 150, "Q", matched=matched)
        got = (outs[True] / "Q-g.variants.hits.tsv").read_bytes()
        assert got == want
        assert len(_table(got)) == int((values[0] > 0).sum()) > 0
        if status:
            assert b"\tlost\t" not in got
            assert b"\tlost\tA\tC\tNA" in (outs[True] / "Q-g.variants.tsv").read_bytes()
