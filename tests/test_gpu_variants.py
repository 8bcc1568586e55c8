"""Variants scored by the triplex potential through them, on the GPU (fasim_score_variants, k_touch, `fasim --variants`): exact
equality of values, encodings and flags with the numpy restatement (test_variants_cpu.py, which never calls the code under test)
over the query lengths at which the kernel takes another path and the kinds and places of variants; the whole-window tie to the
peaks of fasim_scan_records_track; independence of the other variants, their order and the launches; refusals; the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_gpu_oligos import _pre_image
from test_track_cpu import enabled_encodings
from test_variants_cpu import expected_scores

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")
LDS_ROWS = 8192          # TOUCH_LDS_ROWS (csrc/kernels.h): longer queries keep their row state in HBM


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    return mod.Engine(0)


def _h19(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]


def _query(golden_dir, m: int) -> bytes:
    h19 = _h19(golden_dir)
    if m <= len(h19):
        return h19[:m] if m == len(h19) else h19[200:200 + m]
    return (h19 * (m // len(h19) + 1))[:m]


def _records(query: bytes, p, seed: int):
    """A 3 kb record with an N run and, across the variants at 1000 and 1200, gapped pre-images of a stretch of the query under the
    first forward and the first reversed enabled encoding (so that a variant there breaks a real site); and a 500-nt record."""
    rng = np.random.default_rng(seed)
    dna = bytearray(synth.random_dna(3000, seed))
    encs = enabled_encodings(p)
    piece = query[:min(len(query), 60)]
    for at, enc in ((1000, encs[0]), (1200, next(e for e in encs if e & 1))):
        pre = bytearray(_pre_image(piece, enc, rng))
        if len(pre) > 20:
            pre[len(pre) // 3:len(pre) // 3] = b"CA"          # a DNA-side insertion
        a = max(0, at - len(pre) // 2)
        dna[a:a + len(pre)] = pre
    dna[2000:2040] = b"N" * 40
    return [bytes(dna[:3000]), synth.random_dna(500, seed + 1)]


def _other(letters: bytes) -> str:
    return bytes({65: 67, 67: 71, 71: 84, 84: 65, 78: 65}[c] for c in letters).decode()


def _variants(mod, dnas):
    """An SNV, an MNV, an insertion (1 -> 5), a deletion (6 -> 1), at record offset 0, on the last base, inside the N run, an
    unusable entry, and an SNV in the middle of the short record."""
    d, V = dnas[0], mod.Variant

    def ref(a, n):
        return d[a:a + n].decode()
    return [V(1, "c", 1000, "snv", ref(1000, 1), _other(d[1000:1001])),
            V(2, "c", 1200, "mnv", ref(1200, 3), _other(d[1200:1203])),
            V(3, "c", 1400, "ins", ref(1400, 1), ref(1400, 1) + "GAGA"),
            V(4, "c", 1600, "del", ref(1600, 6), ref(1600, 1)),
            V(5, "c", 0, "first", ref(0, 1), _other(d[0:1])),
            V(6, "c", 2999, "last", ref(2999, 1), _other(d[2999:3000])),
            V(7, "c", 2020, "inN", "N", "A"),
            V(8, "c", 1500, "sym", ref(1500, 1), "<DEL>", 0, False),
            V(9, "d", 250, "short", dnas[1][250:251].decode(), _other(dnas[1][250:251]), 1)]


def _check(eng, query, dnas, variants, flank, p, what):
    values, encs, flags = eng.score_variants(variants, dnas, p, flank=flank, queries=[query])
    want = expected_scores(query, dnas, variants, flank, p)
    for got, exp, name in zip((values[0], encs[0], flags[0]), want, ("values", "encs", "flags")):
        got, exp = np.asarray(got, dtype=np.int64), np.asarray(exp, dtype=np.int64)
        assert got.shape == exp.shape, (what, name, got.shape, exp.shape)
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, (what, name, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]))
    return want


@pytest.mark.parametrize("m", [1, 20, 64, 65, 112, 113, 128, 129, 255, 256, 257, 700])
def test_query_lengths_equal_the_restatement(mod, eng, golden_dir, m):
    """Both sides of the steps between workgroups of 64, 128 and 256 threads; one row per thread, threads without rows, exactly 256
    rows, two rows for the first threads and none for the last, three rows per thread."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, m)
    dnas = _records(query, p, 100 + m)
    values, _, _ = _check(eng, query, dnas, _variants(mod, dnas), 300, p, f"m={m}")
    assert values[7].max() == 0 and values[:7].max() > 0


def test_h19_equals_the_restatement(mod, eng, golden_dir):
    p = mod.default_params(rule=1)
    query = _h19(golden_dir)
    assert len(query) == 2812
    dnas = _records(query, p, 7)
    _check(eng, query, dnas, _variants(mod, dnas)[:5], 300, p, "H19")


@pytest.mark.parametrize("m", [LDS_ROWS, LDS_ROWS + 1])
def test_both_sides_of_the_lds_boundary(mod, eng, golden_dir, m):
    """The longest query whose row state lives in LDS and the shortest whose row state lives in HBM; rule 1 and one strand: two
    encodings."""
    p = mod.default_params(rule=1, strand=1)
    assert enabled_encodings(p) == [0, 1]
    query = _query(golden_dir, m)
    dnas = _records(query, p, 11)
    _check(eng, query, dnas, _variants(mod, dnas)[:2], 300, p, f"m={m}")


def test_longest_query(mod, eng, golden_dir):
    """FASIM_MAX_QUERY rows (361 per thread, row state in HBM), one SNV, flank 50, two encodings."""
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, mod.MAX_QUERY)
    dnas = _records(query, p, 13)
    _check(eng, query, dnas, _variants(mod, dnas)[:1], 50, p, "m=MAX_QUERY")


@pytest.mark.parametrize("flank", [300, 0, 10, 2048])
def test_all_48_encodings_and_the_flanks(mod, eng, golden_dir, flank):
    """flank 0: the window is the allele alone; flank 10: the planted sites run past the window, other alignments end inside it
    (clipped and unclipped variants in one call); flank 2048: larger than the short record, and the windows of the long one end at the
    record's ends on one side or both."""
    p = mod.default_params()
    assert len(enabled_encodings(p)) == 48
    query = _query(golden_dir, 40)
    dnas = _records(query, p, 21)
    _, encs, flags = _check(eng, query, dnas, _variants(mod, dnas), flank, p, f"flank={flank}")
    if flank == 300:
        assert len(set(encs[encs >= 0].tolist())) >= 8
    if flank == 0:
        assert flags[:4].all()                               # every alignment of a window that is all allele reaches a cut end
    if flank == 10:
        assert flags.any() and not flags.all()
    if flank == 2048:
        assert not flags[[0, 1, 2, 3, 8]].any()              # their windows are whole records: no end is cut by the flank


def _end_cases(mod, golden_dir):
    """(20-nt query, a 301-nt record with pre-images of the query on its first and its last letters, an SNV, an insertion and a
    deletion at position 0 and the same three ending on the record's last letter): windows with an empty side."""
    p = mod.default_params()
    query = _query(golden_dir, 20)
    rng = np.random.default_rng(27)
    rec = bytearray(synth.random_dna(301, 27))
    encs = enabled_encodings(p)
    head, tail = _pre_image(query, encs[0], rng), _pre_image(query, next(e for e in encs if e & 1), rng)
    rec[:len(head)] = head
    rec[len(rec) - len(tail):] = tail
    rec, n, V = bytes(rec), len(rec), mod.Variant

    def ref(a, k):
        return rec[a:a + k].decode()
    variants = [V(1, "c", 0, "snv0", ref(0, 1), _other(rec[0:1])),
                V(2, "c", 0, "ins0", ref(0, 1), ref(0, 1) + "GA"),
                V(3, "c", 0, "del0", ref(0, 4), ref(0, 1)),
                V(4, "c", n - 1, "snvN", ref(n - 1, 1), _other(rec[n - 1:n])),
                V(5, "c", n - 1, "insN", ref(n - 1, 1), ref(n - 1, 1) + "GA"),
                V(6, "c", n - 4, "delN", ref(n - 4, 4), ref(n - 4, 1))]
    return query, rec, variants, p


@pytest.mark.parametrize("flank", [0, 10])
def test_windows_with_an_empty_side(mod, golden_dir, flank):
    """Variants on the record's first and last letters: the window has no left or no right side (with flank 0 neither: the allele is
    the whole window), so it is two pieces or one.  All 48 encodings, streamed and resident, equal to the restatement."""
    query, rec, variants, p = _end_cases(mod, golden_dir)
    assert len(enabled_encodings(p)) == 48
    e = mod.Engine(0)
    want = _check(e, query, [rec], variants, flank, p, f"streamed, flank={flank}")
    assert want[0][:3].max() > 0 and want[0][3:].max() > 0
    streamed = e.score_variants(variants, [rec], p, flank=flank, queries=[query])
    e.load_dna(rec)
    resident = e.score_variants(variants, None, p, flank=flank, queries=[query])
    for a, b in zip(streamed, resident):
        assert np.array_equal(a, b)
    assert e.last_variant_stats["problems"] == 2 * 48 * len(variants)
    e.close()


def test_resident_record_and_several_queries(mod, golden_dir):
    e = mod.Engine(0)
    p = mod.default_params(rule=2)
    queries = [_query(golden_dir, 33), _query(golden_dir, 300)]
    dnas = _records(queries[1], p, 31)
    variants = [v for v in _variants(mod, dnas) if v.rec == 0]
    streamed = e.score_variants(variants, [dnas[0]], p, flank=100, queries=queries)
    e.load_dna(dnas[0])
    resident = e.score_variants(variants, None, p, flank=100, queries=queries)
    for a, b in zip(streamed, resident):
        assert np.array_equal(a, b)
    for q, query in enumerate(queries):
        want = expected_scores(query, dnas, variants, 100, p)
        assert np.array_equal(streamed[0][q], want[0]) and np.array_equal(streamed[1][q], want[1]) and np.array_equal(streamed[2][q], want[2])
    assert e.last_variant_stats["problems"] == 2 * len(queries) * 4 * sum(v.usable for v in variants)
    e.close()


def test_whole_window_equals_the_peak_of_the_record(mod, golden_dir):
    """A 600-nt record whose REF is the whole record, flank 0: the mark is the whole window, so each class's ref value is the
    record's peak of fasim_scan_records_track (bin 0) with H19 (the pad rows of the scan only repeat values of the real rows)."""
    e = mod.Engine(0)
    rec = synth.random_dna(600, 600)
    assert len(set(rec)) == 4
    h19 = _h19(golden_dir)
    e.set_query(h19)
    p = mod.default_params()
    alt = rec[:300] + _other(rec[300:301]).encode() + rec[301:]
    values, encs, flags = e.score_variants([mod.Variant(1, "c", 0, "all", rec.decode(), alt.decode())], [rec], p, flank=0)
    _, _, peaks = e.scan_records_track([rec], p, bin=0, records=False)
    assert peaks.shape == (1, 4, 3) and 0 < peaks[0, :, 0].max() < 16383
    assert values[0, 0, 0].tolist() == peaks[0, :, 0].tolist()
    assert flags[0, 0] == 0                                  # both ends are the record's
    e.close()


def test_independent_of_the_other_variants_their_order_and_the_launches(mod, golden_dir):
    """700 variants x 2 alleles x 48 encodings = 67 200 problems of about 600 target codes: 40 MB, more than the 16 MB of target
    codes one launch takes.  The engine's own query and a following plain scan are untouched."""
    e = mod.Engine(0)
    h19 = _h19(golden_dir)
    dna = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    e.set_query(h19)
    p = mod.default_params(cLength=40)
    before = e.scan(dna, p)
    oligo = _query(golden_dir, 20)
    rec = synth.random_dna(3000, 5)
    rng = np.random.default_rng(9)
    variants = []
    for k in range(700):
        a = int(rng.integers(0, 2990))
        kind = k % 3
        ref = rec[a:a + (1, 1, 4)[kind]].decode()
        alt = (_other(ref.encode()), ref + "TC", ref[0])[kind]
        variants.append(mod.Variant(k + 1, "c", a, f"v{k}", ref, alt))
    pv = mod.default_params()
    values, encs, flags = e.score_variants(variants, [rec], pv, flank=300, queries=[oligo])
    assert e.last_variant_stats["problems"] == 700 * 96
    assert values.max() > 0
    perm = rng.permutation(700)
    v2, e2, f2 = e.score_variants([variants[i] for i in perm], [rec], pv, flank=300, queries=[oligo])
    assert np.array_equal(v2[0], values[0][perm]) and np.array_equal(e2[0], encs[0][perm]) and np.array_equal(f2[0], flags[0][perm])
    for i in perm[:7]:
        v1, e1, f1 = e.score_variants([variants[i]], [rec], pv, flank=300, queries=[oligo])
        assert np.array_equal(v1[0, 0], values[0, i]) and np.array_equal(e1[0, 0], encs[0, i]) and f1[0, 0] == flags[0, i]
    assert e.rna == h19
    after = e.scan(dna, p)
    assert after.recs == before.recs and after.pool == before.pool
    e.close()


def test_refusals_leave_the_engine_usable(mod, eng, golden_dir):
    V = mod.Variant
    rec = synth.random_dna(200, 3)
    q = _query(golden_dir, 30)
    p = mod.default_params(rule=1)
    ok = V(1, "c", 50, ".", rec[50:51].decode(), "A" if rec[50:51] != b"A" else "C")
    cases = [
        (dict(variants=[V(1, "c", 200, ".", "A", "C")]), mod.E_ARG),                    # outside its record
        (dict(variants=[V(1, "c", 198, ".", "ACG", "C")]), mod.E_ARG),                  # REF runs past the record's end
        (dict(variants=[V(1, "c", -1, ".", "A", "C")]), mod.E_ARG),
        (dict(variants=[V(1, "c", 5, ".", "A", "C", 1)]), mod.E_ARG),                   # no such record
        (dict(variants=[V(1, "c", 5, ".", "", "C")]), mod.E_ARG),                       # ref_len < 1
        (dict(variants=[V(1, "c", 5, ".", "A", "")]), mod.E_ARG),
        (dict(variants=[V(1, "c", 5, ".", "A", "C" * (mod.MAX_ALLELE + 1))]), mod.E_ARG),
        (dict(flank=-1), mod.E_ARG),
        (dict(flank=mod.MAX_FLANK + 1), mod.E_ARG),
        (dict(queries=[b"A" * (mod.MAX_QUERY + 1)]), mod.E_UNSUPPORTED),
        (dict(p=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED),
    ]
    for kw, code in cases:
        args = dict(variants=[ok], dnas=[rec], p=p, flank=20, queries=[q])
        args.update(kw)
        with pytest.raises(mod.FasimError) as ei:
            eng.score_variants(**args)
        assert ei.value.code == code, (kw.keys(), str(ei.value))
    _check(eng, q, [rec], [ok], 20, p, "after the refusals")


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_table_equals_the_python_results(mod, eng, tmp_path, golden_dir):
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
    good = [f"chr1\t1001\trs1\t{ref(chr1, 1001)}\t{_other(chr1[1000:1001])}\t.\tPASS\n",
            f"chr1\t1201\trs2\t{ref(chr1, 1201, 2)}\t{ref(chr1, 1201)},{ref(chr1, 1201, 2)}GG\n",
            f"chr2\t251\trs3\t{ref(chr2, 251).lower()}\t{_other(chr2[250:251]).lower()}\n",
            f"chr1\t3000\trs4\t{ref(chr1, 3000)}\t{_other(chr1[2999:3000])}\n"]
    bad = [f"chr1\t501\tmism\t{_other(chr1[500:501])}\t{ref(chr1, 501)}\n",
           f"chr1\t601\tstar\t{ref(chr1, 601)}\t*\n",
           "chr7\t10\tlost\tA\tC\n",
           f"chr2\t500\tpast\t{ref(chr2, 500)}A\tC\n"]
    lines = ["##fileformat=VCFv4.2\n", "#CHROM\tPOS\tID\tREF\tALT\n", good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3], bad[3]]
    for name, text, status in (("all.vcf", "".join(lines), 1), ("good.vcf", "".join(lines[:2] + good), 0)):
        (tmp_path / name).write_text(text)
        out = tmp_path / ("out_" + name)
        out.mkdir()
        r = subprocess.run([EXE, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--variants", name, "--variant-flank", "150"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == status, r.stderr
        assert sorted(os.listdir(out)) == ["Q-g.variants.tsv"]
        variants = [v._replace(rec=1 if v.chrom == "chr2" else 0) for v in mod.read_vcf(str(tmp_path / name))]
        matched = [v.usable and v.id.startswith("rs") for v in variants]
        score = [v if ok else v._replace(usable=False) for v, ok in zip(variants, matched)]
        values, encs, flags = eng.score_variants(score, dnas, p, flank=150, queries=[q])
        want = mod.variants_tsv(variants, values[0], encs[0], flags[0], 150, "Q", matched=matched)
        assert (out / "Q-g.variants.tsv").read_bytes() == want
        if status:
            for word in ("REF differs", "cannot be scored", "no DNA record of its chromosome", "contains it", "4 of 9 variants"):
                assert word in r.stderr, r.stderr
            assert "VCF line 4 chr1:501: REF differs" in r.stderr
        else:
            assert "finished normally" in r.stdout
