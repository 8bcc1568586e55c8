"""Every SNV of an interval from one shared pass, on the GPU (fasim_score_mutagenesis; k_mut_prefix, k_mut_touch, k_mut_reduce;
`fasim --mutagenesis`): exact equality of values, encodings, ref, clip bits and of the call's cont_cols -- the columns the problems
ran until their dead column -- with the numpy restatement (test_mutagenesis_cpu.py, which never calls the code under test) over the
query lengths at which the kernels take another path, all encodings, the context's ends, the early stop and odd letters; equality
with fasim_score_variants on the cut-out context; independence of the other intervals, their order and the launches; refusals; the
CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_gpu_oligos import _pre_image
from test_gpu_variants import LDS_ROWS, _h19, _query, _records
from test_mutagenesis_cpu import ACGT, context, expected_mutagenesis, touch_life
from test_track_cpu import enabled_encodings, encode_unit

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    return mod.Engine(0)


def _check(eng, query, dnas, intervals, flank, p, what):
    """One call against the restatement, interval by interval; returns (values, encs, ref, clipped) of the call for the query."""
    values, encs, ref, clipped, offsets = eng.score_mutagenesis(intervals, dnas, p, flank=flank, queries=[query])
    st = eng.last_mutagenesis_stats
    assert offsets.tolist() == np.cumsum([0] + [e - s for _, s, e in intervals]).tolist()
    cont = bound = 0
    for k, (rec, start, end) in enumerate(intervals):
        ev, ee, er, ec, info = expected_mutagenesis(query, dnas[rec], start, end, flank, p)
        a, b = int(offsets[k]), int(offsets[k + 1])
        for got, exp, name in ((values[0, a:b], ev, "values"), (encs[0, a:b], ee, "encs"), (ref[a:b], er, "ref"), (clipped[0, a:b], ec, "clipped")):
            got, exp = np.asarray(got, dtype=np.int64), np.asarray(exp, dtype=np.int64)
            assert got.shape == exp.shape, (what, k, name, got.shape, exp.shape)
            bad = np.argwhere(got != exp)
            assert len(bad) == 0, (what, k, name, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]))
        cont += info["cont_cols"]
        bound += info["cont_cols_bound"]
    print(f"{what}: cont_cols {st['cont_cols']} (restatement {cont}) of {st['cont_cols_bound']} (restatement {bound})")
    assert st["cont_cols"] == cont and st["cont_cols_bound"] == bound, (what, st, cont, bound)
    nenc = len(enabled_encodings(p))
    assert st["positions"] == int(offsets[-1]) and st["problems"] == 4 * nenc * st["positions"] and st["intervals"] == len(intervals)
    return values[0], encs[0], ref, clipped[0]


# ---- query lengths and planted sites -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 20, 64, 65, 128, 129, 256, 257, 700])
def test_query_lengths_equal_the_restatement(mod, eng, golden_dir, m):
    """Both sides of the steps between workgroups of 64, 128 and 256 threads, one to three rows per thread, threads without rows.
    Two 24-position intervals of test_gpu_variants' record, across its planted gapped pre-images under the first forward and the
    first reversed encoding, flank 16."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, m)
    dnas = _records(query, p, 100 + m)
    values, _, ref, _ = _check(eng, query, dnas, [(0, 988, 1012), (0, 1188, 1212)], 16, p, f"m={m}")
    assert values.max() > 0 and (ref >= 0).all()
    if m >= 20:      # a letter matters somewhere: the four letters of a position do not all have the same values
        assert (values.max(axis=1) > values.min(axis=1)).any()


# ---- the LDS boundary and the longest query ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [LDS_ROWS, LDS_ROWS + 1])
def test_both_sides_of_the_lds_boundary(mod, eng, golden_dir, m):
    """The longest query whose row state lives in LDS and the shortest whose row state and snapshots' target live in HBM; two
    encodings, 6 positions, flank 8."""
    p = mod.default_params(rule=1, strand=1)
    assert enabled_encodings(p) == [0, 1]
    query = _query(golden_dir, m)
    dnas = _records(query, p, 11)
    values, _, _, _ = _check(eng, query, dnas, [(0, 997, 1003)], 8, p, f"m={m}")
    assert values.max() > 0


def test_longest_query(mod, eng, golden_dir):
    """FASIM_MAX_QUERY rows (361 per thread, row state in HBM), two encodings, 2 positions, flank 8."""
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, mod.MAX_QUERY)
    dnas = _records(query, p, 13)
    _check(eng, query, dnas, [(0, 999, 1001)], 8, p, "m=MAX_QUERY")


# ---- encodings and context ends ---------------------------------------------------------------------------------------------------
def _short_record(query, p, n, seed, at):
    """n nt of random DNA with gapped pre-images of the query's first letters under the first forward and the first reversed
    encoding, centred on the offsets `at`."""
    rng = np.random.default_rng(seed)
    dna = bytearray(synth.random_dna(n, seed))
    encs = enabled_encodings(p)
    for a, enc in zip(at, (encs[0], next(e for e in encs if e & 1))):
        pre = bytearray(_pre_image(query[:min(len(query), 30)], enc, rng))
        if len(pre) > 20:
            pre[len(pre) // 3:len(pre) // 3] = b"CA"
        a = max(0, a - len(pre) // 2)
        dna[a:a + len(pre)] = pre
    return bytes(dna[:n])


def test_all_48_encodings_on_an_asymmetric_context(mod, eng, golden_dir):
    """Start 5, flank 40: the context has 5 letters before the interval and 40 behind it, so a mirror taken about the wrong centre
    lands outside the interval."""
    p = mod.default_params()
    assert len(enabled_encodings(p)) == 48
    query = _query(golden_dir, 40)
    dna = _short_record(query, p, 200, 51, (8, 30))
    _, encs, _, _ = _check(eng, query, [dna], [(0, 5, 11)], 40, p, "48 encodings")
    assert (encs[encs >= 0] & 1).any() and (~encs[encs >= 0] & 1).any() and encs.max() >= 12


def test_context_ends(mod, eng, golden_dir):
    """start = 0, end = the record's length, flank 0, flank 2048 on a 500-nt record, one position, an interval that is its whole
    record.  Where an end is cut by the flank clipped and unclipped letters both occur; where both ends are record ends none is
    clipped."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 40)
    dna = _short_record(query, p, 500, 61, (4, 494))
    small = _short_record(query, p, 60, 62, (20, 40))
    cut, whole = [], []
    for what, dnas, iv, flank, is_cut in (("start 0", [dna], (0, 0, 10), 16, True), ("end at the record's", [dna], (0, 490, 500), 16, True),
                                          ("flank 0", [dna], (0, 2, 10), 0, True), ("flank 2048", [dna], (0, 240, 250), 2048, False),
                                          ("one position", [dna], (0, 250, 251), 16, True), ("the whole record", [small], (0, 0, 60), 5, False)):
        _, _, _, clipped = _check(eng, query, dnas, [iv], flank, p, what)
        (cut if is_cut else whole).append(clipped)
    cut, whole = np.concatenate(cut), np.concatenate(whole)
    assert cut.any() and not cut.all()
    assert not whole.any()


# ---- the early stop ---------------------------------------------------------------------------------------------------------------
def test_early_stop_on_random_dna(mod, eng, golden_dir):
    """A 20-nt oligo, flank 300, all 48 encodings: the problems die long before the context's end."""
    p = mod.default_params()
    query = _query(golden_dir, 20)
    dna = synth.random_dna(2000, 71)
    _check(eng, query, [dna], [(0, 1000, 1008)], 300, p, "random DNA")
    st = eng.last_mutagenesis_stats
    assert st["cont_cols"] * 2 < st["cont_cols_bound"]
    assert st["prefix_problems"] == 48 and st["prefix_cols"] == 48 * 307 and st["launches"] == 1


def test_a_site_to_the_cut_end_keeps_its_problems_alive(mod, eng):
    """A perfect 60-mer under encoding 0 from inside the interval to the context's cut end: the problems through it with the
    record's own letter run to column n - 1 and carry the clip bit."""
    p = mod.default_params(rule=1, strand=1)
    rng = np.random.default_rng(5)
    query = bytes(rng.choice(np.frombuffer(b"TG", dtype=np.uint8), 60))
    pre = query.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A")
    assert encode_unit(pre, 0) == query
    dna = synth.random_dna(300, 72) + pre + synth.random_dna(300, 73)
    start, end, flank = 302, 306, 54
    lo, hi, e_lo, e_hi = context(dna, start, end, flank)
    assert hi == 360 and e_hi
    n = hi - lo
    words, ran = touch_life(query, [encode_unit(dna[lo:hi], 0)] * 4, [x - lo for x in range(start, end)], e_lo, e_hi)
    assert ran.tolist() == [n - (x - lo) for x in range(start, end)] and (words & 1).all()
    values, encs, ref, clipped = _check(eng, query, [dna], [(0, start, end)], flank, p, "planted 60-mer")
    own = np.arange(4), ref
    assert (clipped[own] == 1).all() and (encs[own][:, 0] == 0).all() and (values[own][:, 0] == 5 * 60).all()


# ---- odd letters ------------------------------------------------------------------------------------------------------------------
def test_odd_letters_in_the_context_and_at_positions(mod, eng, golden_dir):
    """N, lower case and IUPAC bytes: ref is -1 there and the four letters are still scored as the restatement scores them."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 40)
    dna = bytearray(_short_record(query, p, 300, 81, (100, 130)))
    dna[90:93] = b"NNN"
    dna[104:107] = b"acg"
    dna[110:112] = b"RY"
    dna[113:114] = b"n"
    dna[140:150] = b"NNNNNNNNNN"
    dna = bytes(dna)
    _, _, ref, _ = _check(eng, query, [dna], [(0, 100, 116)], 30, p, "odd letters")
    want = [ACGT.find(dna[x:x + 1]) for x in range(100, 116)]
    assert ref.tolist() == want and want.count(-1) == 6


# ---- against the existing product on the device ------------------------------------------------------------------------------------
def test_equals_score_variants_on_the_cut_out_context(mod, eng, golden_dir):
    """Every SNV of a 30-position interval, context of 2 030 letters: values and encodings are those of score_variants for the SNV
    on the record dna[lo:hi] with flank 2048, whose window is the whole context."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 300)
    dnas = _records(query, p, 91)
    start, end, flank = 1185, 1215, 1000      # across the pre-image planted under the reversed encoding
    lo, hi, _, _ = context(dnas[0], start, end, flank)
    assert hi - lo == 2030
    values, encs, ref, _, _ = eng.score_mutagenesis([(0, start, end)], dnas, p, flank=flank, queries=[query])
    snvs = [(x, b) for x in range(start, end) for b in range(4) if b != ref[x - start]]
    assert len(snvs) == 90
    variants = [mod.Variant(1, "c", x - lo, ".", chr(dnas[0][x]), chr(ACGT[b])) for x, b in snvs]
    v, e, _ = eng.score_variants(variants, [dnas[0][lo:hi]], p, flank=2048, queries=[query])
    for k, (x, b) in enumerate(snvs):
        j, r = x - start, int(ref[x - start])
        assert values[0, j, b].tolist() == v[0, k, 1].tolist() and encs[0, j, b].tolist() == e[0, k, 1].tolist(), (x, b)
        assert values[0, j, r].tolist() == v[0, k, 0].tolist() and encs[0, j, r].tolist() == e[0, k, 0].tolist(), (x, b)
    assert values.max() > 0
    assert [tuple(t)[2:6] for t in mod.mutagenesis_variants([(0, start, end)], dnas)] == [(x, ".", chr(dnas[0][x]), chr(ACGT[b])) for x, b in snvs]


# ---- independence -----------------------------------------------------------------------------------------------------------------
def test_independent_of_the_other_intervals_their_order_and_the_engine(mod, golden_dir):
    """Overlapping, nested and repeated intervals on two records, two queries; permuted; one by one.  The engine's own query and a
    plain scan before and after are untouched, and a resident record gives what a passed one gives."""
    e = mod.Engine(0)
    h19 = _h19(golden_dir)
    demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    e.set_query(h19)
    ps = mod.default_params(cLength=40)
    before = e.scan(demo, ps)
    p = mod.default_params(rule=2)
    queries = [_query(golden_dir, 33), _query(golden_dir, 300)]
    dnas = _records(queries[1], p, 31)
    ivs = [(0, 990, 1010), (0, 1000, 1030), (0, 1002, 1006), (1, 240, 250), (0, 990, 1010), (0, 0, 3), (1, 495, 500)]
    values, encs, ref, clipped, offsets = e.score_mutagenesis(ivs, dnas, p, flank=100, queries=queries)
    assert values.shape == (2, int(offsets[-1]), 4, 4) and clipped.shape == (2, int(offsets[-1]), 4) and values.max() > 0
    perm = [3, 6, 0, 5, 2, 4, 1]
    v2, e2, r2, c2, o2 = e.score_mutagenesis([ivs[k] for k in perm], dnas, p, flank=100, queries=queries)
    for at, k in enumerate(perm):
        a, b, a2, b2 = int(offsets[k]), int(offsets[k + 1]), int(o2[at]), int(o2[at + 1])
        assert np.array_equal(v2[:, a2:b2], values[:, a:b]) and np.array_equal(e2[:, a2:b2], encs[:, a:b])
        assert np.array_equal(r2[a2:b2], ref[a:b]) and np.array_equal(c2[:, a2:b2], clipped[:, a:b])
    for k, iv in enumerate(ivs):
        a, b = int(offsets[k]), int(offsets[k + 1])
        for q in range(2):
            v1, e1, r1, c1, _ = e.score_mutagenesis([iv], dnas, p, flank=100, queries=[queries[q]])
            assert np.array_equal(v1[0], values[q, a:b]) and np.array_equal(e1[0], encs[q, a:b])
            assert np.array_equal(r1, ref[a:b]) and np.array_equal(c1[0], clipped[q, a:b])
    assert np.array_equal(values[:, offsets[0]:offsets[1]], values[:, offsets[4]:offsets[5]])
    e.load_dna(dnas[0])
    res = e.score_mutagenesis([iv for iv in ivs if iv[0] == 0], None, p, flank=100, queries=queries)
    keep = np.concatenate([np.arange(offsets[k], offsets[k + 1]) for k, iv in enumerate(ivs) if iv[0] == 0])
    assert np.array_equal(res[0], values[:, keep]) and np.array_equal(res[1], encs[:, keep]) and np.array_equal(res[3], clipped[:, keep])
    assert e.rna == h19
    after = e.scan(demo, ps)
    assert after.recs == before.recs and after.pool == before.pool
    e.close()


def test_independent_of_the_launches(mod, eng, golden_dir):
    """A 20-nt oligo under 48 encodings has 192 problems per position, and a launch takes 2^20 problems: 5 461 positions.  Two
    intervals of 5 120 and 400 positions (flank 0) are cut into two launches, the cut inside the second interval; each interval alone
    is one launch."""
    p = mod.default_params()
    query = _query(golden_dir, 20)
    dna = synth.random_dna(5600, 95)
    ivs = [(0, 0, 5120), (0, 5100, 5500)]
    values, encs, ref, clipped, offsets = eng.score_mutagenesis(ivs, [dna], p, flank=0, queries=[query])
    assert eng.last_mutagenesis_stats["launches"] == 2 and eng.last_mutagenesis_stats["prefix_problems"] == 3 * 48
    for k, iv in enumerate(ivs):
        a, b = int(offsets[k]), int(offsets[k + 1])
        v1, e1, r1, c1, _ = eng.score_mutagenesis([iv], [dna], p, flank=0, queries=[query])
        assert eng.last_mutagenesis_stats["launches"] == 1
        assert np.array_equal(v1[0], values[0, a:b]) and np.array_equal(e1[0], encs[0, a:b])
        assert np.array_equal(r1, ref[a:b]) and np.array_equal(c1[0], clipped[0, a:b])
    assert values.max() > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mod, eng, golden_dir):
    rec = synth.random_dna(6000, 3)
    q = _query(golden_dir, 30)
    p = mod.default_params(rule=1)
    cases = [
        (dict(intervals=[(0, 5990, 6001)]), mod.E_ARG),                     # runs past its record's end
        (dict(intervals=[(0, -1, 5)]), mod.E_ARG),
        (dict(intervals=[(0, 5, 5)]), mod.E_ARG),                           # no position
        (dict(intervals=[(1, 0, 5)]), mod.E_ARG),                           # no such record
        (dict(intervals=[(0, 0, 5081)]), mod.E_ARG),                        # 5 081 + 2 * 20 > 5 120
        (dict(intervals=[(0, 0, 1025)], flank=2048), mod.E_ARG),
        (dict(flank=-1), mod.E_ARG),
        (dict(flank=mod.MAX_FLANK + 1), mod.E_ARG),
        (dict(queries=[b"A" * (mod.MAX_QUERY + 1)]), mod.E_UNSUPPORTED),
        (dict(queries=[b""]), mod.E_ARG),
        (dict(p=mod.default_params(classicSim=1)), mod.E_UNSUPPORTED),
    ]
    for kw, code in cases:
        args = dict(intervals=[(0, 50, 54)], dnas=[rec], p=p, flank=20, queries=[q])
        args.update(kw)
        with pytest.raises(mod.FasimError) as ei:
            eng.score_mutagenesis(**args)
        assert ei.value.code == code, (kw.keys(), str(ei.value))
    _check(eng, q, [rec], [(0, 50, 54)], 20, p, "after the refusals")
    eng.score_mutagenesis([(0, 0, 5080)], [rec], p, flank=20, queries=[q[:4]])      # the widest context there is


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_table_equals_the_python_results(mod, eng, tmp_path, golden_dir):
    q = _query(golden_dir, 60)
    p = mod.default_params()
    dnas = _records(q, p, 41)
    chr1, chr2 = dnas
    chr1 = chr1[:995] + b"n" + chr1[996:]                                  # a position without lines
    dnas = [chr1, chr2]
    synth.write_fasta(str(tmp_path / "g.fa"), "chr1 test record", chr1)
    with open(tmp_path / "g.fa", "a") as f:
        f.write(">chr2\n" + chr2.decode() + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + q.decode() + "\n")
    good = ["chr1\t990\t1010\tsite\n", "chr2\t495\t500\n", "chr1\t1195\t1205\tsite\n"]
    bad = ["chr7\t10\t20\tlost\n", "chr2\t495\t501\tpast\n"]
    for name, lines, status in (("all.bed", ["# intervals\n", good[0], bad[0], good[1], bad[1], good[2]], 1), ("good.bed", good, 0)):
        (tmp_path / name).write_text("".join(lines))
        out = tmp_path / ("out_" + name)
        out.mkdir()
        r = subprocess.run([EXE, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--mutagenesis", name, "--mutagenesis-flank", "150"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == status, r.stderr
        assert sorted(os.listdir(out)) == ["Q-g.mutagenesis.tsv"]
        regions = mod.read_bed(str(tmp_path / name))
        held = [g for g in regions if g.name not in ("lost", "past")]
        ivs = [(1 if g.chrom == "chr2" else 0, g.start, g.end) for g in held]
        values, encs, ref, clipped, offsets = eng.score_mutagenesis(ivs, dnas, p, flank=150, queries=[q])
        full, at = [0], 0
        for g in regions:
            if g in held:
                at += 1
            full.append(int(offsets[at]))
        want = mod.mutagenesis_tsv(regions, values[0], encs[0], ref, clipped[0], full, 150, "Q")
        got = (out / "Q-g.mutagenesis.tsv").read_bytes()
        assert got == want
        assert got.count(b"\n") == 2 + 3 * (20 - 1 + 5 + 10) and b"\tsite_" in got      # (the second `site` of chr1 is renamed)
        if status:
            for word in ("BED line 3 (lost) chr7:10-20: no DNA record of its chromosome", "BED line 5 (past)", "runs past the end", "2 of 5 BED intervals"):
                assert word in r.stderr, r.stderr
        else:
            assert "finished normally" in r.stdout
