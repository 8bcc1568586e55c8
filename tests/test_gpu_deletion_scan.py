"""Every deletion of an interval from the shared pass, on the GPU (fasim_score_deletions; k_mut_prefix_pm, k_mut_jump,
k_mut_del_reduce; `fasim --mutagenesis --deletions`): exact equality of values, encodings, clip bits, valid and clean with the
definition's restatement expected_deletions, and of the call's counters -- own-letter and ALT problems, the columns they ran until
their dead column, the bound -- with jump_life (both in test_deletion_scan_cpu.py, neither calls the code under test), over the query
lengths at which the kernels take another path, all encodings, the context's ends, planted sites, the early stop and odd letters;
equality with fasim_score_variants on the cut-out context; independence of the other intervals, their order, the launches and of
score_mutagenesis; refusals; the CLI.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_deletion_scan_cpu import deletions_of, early_stop_case, expected_deletions, jump_life
from test_gpu_mutagenesis import _short_record
from test_gpu_oligos import _pre_image
from test_gpu_variants import LDS_ROWS, _h19, _query, _records
from test_mutagenesis_cpu import context
from test_track_cpu import enabled_encodings, encode_unit

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")
COUNTERS = ("own_problems", "alt_problems", "cont_cols", "cont_cols_bound")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    return mod.Engine(0)


def _check(eng, query, dnas, intervals, flank, lengths, p, what):
    """One call against the restatements, interval by interval (each interval is one group of one launch here); returns (values,
    encs, clipped, valid, clean) of the call for the query."""
    values, encs, clipped, valid, clean, offsets = eng.score_deletions(intervals, dnas, p, flank=flank, lengths=lengths, queries=[query])
    st = eng.last_deletion_stats
    assert offsets.tolist() == np.cumsum([0] + [e - s for _, s, e in intervals]).tolist()
    assert values.shape == (1, int(offsets[-1]), len(lengths), 2, 4) and clipped.shape == (1, int(offsets[-1]), len(lengths), 2)
    want = dict.fromkeys(COUNTERS, 0)
    ndel = 0
    for k, (rec, start, end) in enumerate(intervals):
        ev, ee, ec, evalid, eclean = expected_deletions(query, dnas[rec], start, end, flank, lengths, p)
        a, b = int(offsets[k]), int(offsets[k + 1])
        for got, exp, name in ((values[0, a:b], ev, "values"), (encs[0, a:b], ee, "encs"), (clipped[0, a:b], ec, "clipped"),
                               (valid[a:b], evalid, "valid"), (clean[a:b], eclean, "clean")):
            got, exp = np.asarray(got, dtype=np.int64), np.asarray(exp, dtype=np.int64)
            assert got.shape == exp.shape, (what, k, name, got.shape, exp.shape)
            bad = np.argwhere(got != exp)
            assert len(bad) == 0, (what, k, name, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(exp[tuple(bad[0])]))
        _, info = jump_life(query, dnas[rec], start, end, flank, lengths, p)
        for c in COUNTERS:
            want[c] += info[c]
        ndel += len(deletions_of(start, end, lengths))
    print(f"{what}: " + ", ".join(f"{c} {st[c]} (restatement {want[c]})" for c in COUNTERS))
    assert {c: st[c] for c in COUNTERS} == want, (what, st, want)
    assert st["positions"] == int(offsets[-1]) and st["intervals"] == len(intervals) and st["deletions"] == ndel
    assert st["alt_problems"] == ndel * len(enabled_encodings(p))
    return values[0], encs[0], clipped[0], valid, clean


# ---- query lengths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 20, 64, 65, 128, 129, 256, 257, 700])
def test_query_lengths_equal_the_restatement(mod, eng, golden_dir, m):
    """Both sides of the steps between workgroups of 64, 128 and 256 threads, one to three rows per thread, threads without rows.
    Two 24-position intervals of test_gpu_variants' record, across its planted gapped pre-images under the first forward and the
    first reversed encoding, flank 16, lengths (1, 3, 10)."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, m)
    dnas = _records(query, p, 100 + m)
    values, _, _, valid, _ = _check(eng, query, dnas, [(0, 988, 1012), (0, 1188, 1212)], 16, (1, 3, 10), p, f"m={m}")
    assert values.max() > 0 and valid.sum() == 2 * (23 + 21 + 14)
    if m >= 20:      # a deletion matters somewhere
        assert (values[:, :, 0] != values[:, :, 1]).any()


# ---- the LDS boundary and the longest query ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [LDS_ROWS, LDS_ROWS + 1])
def test_both_sides_of_the_lds_boundary(mod, eng, golden_dir, m):
    """The longest query whose row state lives in LDS and the shortest whose row state lives in HBM; two encodings, 6 positions,
    lengths (1, 4), flank 8."""
    p = mod.default_params(rule=1, strand=1)
    assert enabled_encodings(p) == [0, 1]
    query = _query(golden_dir, m)
    dnas = _records(query, p, 11)
    values, _, _, _, _ = _check(eng, query, dnas, [(0, 997, 1003)], 8, (1, 4), p, f"m={m}")
    assert values.max() > 0


def test_longest_query(mod, eng, golden_dir):
    """FASIM_MAX_QUERY rows (361 per thread, row state in HBM), two encodings, 3 positions, lengths (1,), flank 8."""
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, mod.MAX_QUERY)
    dnas = _records(query, p, 13)
    _check(eng, query, dnas, [(0, 999, 1002)], 8, (1,), p, "m=MAX_QUERY")


# ---- encodings and context ends ---------------------------------------------------------------------------------------------------
def test_all_48_encodings_on_an_asymmetric_context(mod, eng, golden_dir):
    """Start 5, flank 40: the context has 5 letters before the interval and 40 behind it, so a mirror taken about the wrong centre
    lands outside the interval."""
    p = mod.default_params()
    assert len(enabled_encodings(p)) == 48
    query = _query(golden_dir, 40)
    dna = _short_record(query, p, 200, 51, (8, 30))
    _, encs, _, _, _ = _check(eng, query, [dna], [(0, 5, 13)], 40, (1, 2, 6), p, "48 encodings")
    assert (encs[encs >= 0] & 1).any() and (~encs[encs >= 0] & 1).any() and encs.max() >= 12


def flank0_case(mod, golden_dir):
    """A 40-nt query and a 500-nt record with a pre-image of its first 30 letters under the first encoding that ends with the interval [240, 262):
    with flank 0 the deletions (x, d), x + d = 261, end at the context's cut upper end."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 40)
    dna = bytearray(_short_record(query, p, 500, 61, (4, 494)))
    dna[232:262] = _pre_image(query[:30], enabled_encodings(p)[0], np.random.default_rng(63))
    return p, query, bytes(dna), (0, 240, 262), (1, 2, 5)


def test_a_deletion_that_ends_at_the_cut_end_has_the_bit_on_its_anchor(mod, eng, golden_dir):
    """Flank 0 and x + 1 + d = hi: ALT's last column is the anchor's, so every ALT value there is clipped."""
    p, query, dna, iv, lengths = flank0_case(mod, golden_dir)
    values, _, clipped, valid, _ = _check(eng, query, [dna], [iv], 0, lengths, p, "flank 0")
    L = iv[2] - iv[1]
    seen = 0
    for li, d in enumerate(lengths):
        j = L - 1 - d
        assert valid[j, li] and not valid[j + 1, li]
        if values[j, li, 1].max() > 0:
            assert clipped[j, li, 1] == 1
            seen += 1
    assert seen > 0
    assert clipped.any() and not clipped[valid == 1].all()


def test_context_ends(mod, eng, golden_dir):
    """start = 0 (no lower edge), end = the record's end, a whole 60-nt record (no clip bit anywhere), flank 2 048 on a 500-nt record,
    intervals of two positions (one deletion) and of one (none: zeros, and no jump problem in the counters), all 16 lengths at
    once."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 40)
    dna = _short_record(query, p, 500, 61, (4, 494))
    small = _short_record(query, p, 60, 62, (20, 40))
    cut, whole = [], []
    for what, dnas, iv, flank, lengths, is_cut in (
            ("start 0", [dna], (0, 0, 10), 16, (1, 3), True), ("end at the record's", [dna], (0, 490, 500), 16, (1, 3), True),
            ("flank 2048", [dna], (0, 240, 250), 2048, (1, 4), False), ("the whole record", [small], (0, 0, 60), 5, (1, 2, 30), False),
            ("two positions", [dna], (0, 250, 252), 16, (1, 2), True),
            ("16 lengths", [dna], (0, 236, 262), 12, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 19, 22, 25), True)):
        values, _, clipped, valid, _ = _check(eng, query, dnas, [iv], flank, lengths, p, what)
        (cut if is_cut else whole).append(clipped[valid == 1].ravel())
        if what == "two positions":
            assert valid.tolist() == [[1, 0], [0, 0]]
    cut, whole = np.concatenate(cut), np.concatenate(whole)
    assert cut.any() and not cut.all()
    assert not whole.any()
    values, encs, clipped, valid, clean = _check(eng, query, [dna], [(0, 250, 251)], 16, (1, 2), p, "one position")
    st = eng.last_deletion_stats
    assert not values.any() and (encs == -1).all() and not clipped.any() and not valid.any() and not clean.any()
    assert st["own_problems"] == st["alt_problems"] == st["cont_cols"] == st["launches"] == st["deletions"] == 0


def test_the_longest_deletion_of_the_widest_interval(mod, eng, golden_dir):
    """1 024 positions, lengths (1023,), flank 0: exactly one deletion, anchored at the first position."""
    p = mod.default_params(rule=1, strand=1)
    query = _query(golden_dir, 20)
    dna = _short_record(query, p, 1100, 64, (12, 1040))
    values, _, _, valid, _ = _check(eng, query, [dna], [(0, 10, 1034)], 0, (1023,), p, "1 024 positions")
    assert valid.sum() == 1 and valid[0, 0] == 1 and eng.last_deletion_stats["launches"] == 1
    assert not values[1:].any()


# ---- a planted site under encoding 0 ------------------------------------------------------------------------------------------------
def planted_site(extra: bool):
    """(query, dna, start, end): a random 60-mer over TG and its encoding-0 pre-image over AT between 300 nt of random DNA on either
    side; `extra`: a C inserted at offset 30 of the site.  [start, end) is the site."""
    rng = np.random.default_rng(5)
    query = bytes(rng.choice(np.frombuffer(b"TG", dtype=np.uint8), 60))
    pre = query.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A")
    assert encode_unit(pre, 0) == query
    site = pre[:30] + b"C" + pre[30:] if extra else pre
    return query, synth.random_dna(300, 72) + site + synth.random_dna(300, 73), 300, 300 + len(site)


def test_one_base_deletions_of_a_perfect_site(mod, eng):
    """Every 1-base deletion inside the perfect 60-mer: REF 300, and ALT 279 -- 59 pairs and one gap -- for the anchors at offsets 3
    to 52.  Nearer to an end of the site the gap's 16 is not the cheapest way past the deletion: leaving the few pairs beyond it out,
    or shifting them by one where the site repeats a letter, costs less, so ALT lies between 279 and 300 there: the definition's restatement
    gives 300, 291, 282 for the offsets 0 to 2 and 286, 286, 286, 286, 295, 295 for 53 to 58, which are asserted as they are."""
    p = mod.default_params(rule=1, strand=1)
    query, dna, start, end = planted_site(False)
    values, encs, _, valid, _ = _check(eng, query, [dna], [(0, start, end)], 100, (1,), p, "perfect site")
    assert valid[:59, 0].all() and not valid[59, 0]
    assert (values[:59, 0, 0, 0] == 300).all() and (encs[:59, 0, :, 0] == 0).all()
    assert (values[3:53, 0, 1, 0] == 279).all()
    assert values[:3, 0, 1, 0].tolist() == [300, 291, 282] and values[53:59, 0, 1, 0].tolist() == [286, 286, 286, 286, 295, 295]


def test_the_deletion_that_repairs_a_site(mod, eng):
    """One extra base at offset 30 of the site: REF is 284 -- 60 pairs and one gap -- for every deletion inside the site, and the one
    deletion that takes the extra base out gives 300."""
    p = mod.default_params(rule=1, strand=1)
    query, dna, start, end = planted_site(True)
    values, _, _, valid, _ = _check(eng, query, [dna], [(0, start, end)], 100, (1,), p, "site with an extra base")
    assert valid[:60, 0].all()
    assert (values[:60, 0, 0, 0] == 284).all()
    assert values[29, 0, 1, 0] == 300 and (np.delete(values[:60, 0, 1, 0], 29) < 300).all()


# ---- the early stop ---------------------------------------------------------------------------------------------------------------
def test_early_stop_on_random_dna(mod, eng):
    """A 20-nt oligo, flank 300, all 48 encodings: the jump problems die long before the context's end."""
    p = mod.default_params()
    query, dna, iv, flank, lengths = early_stop_case()
    _check(eng, query, [dna], [iv], flank, lengths, p, "random DNA")
    st = eng.last_deletion_stats
    assert st["cont_cols"] * 2 < st["cont_cols_bound"]
    assert st["prefix_problems"] == 48 and st["launches"] == 1


# ---- odd letters ------------------------------------------------------------------------------------------------------------------
def test_odd_letters_in_the_anchor_the_run_and_the_context(mod, eng, golden_dir, tmp_path):
    """N, lower case and IUPAC bytes: scored as the restatement scores them, clean is 0 exactly where one of the d + 1 bytes is
    odd, and the table has no such lines."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 40)
    dna = bytearray(_short_record(query, p, 300, 81, (100, 130)))
    dna[90:93] = b"NNN"
    dna[104:106] = b"ac"
    dna[110:112] = b"RY"
    dna[113:114] = b"n"
    dna[140:150] = b"NNNNNNNNNN"
    dna = bytes(dna)
    start, end, lengths = 100, 118, (1, 3)
    values, encs, clipped, valid, clean = _check(eng, query, [dna], [(0, start, end)], 30, lengths, p, "odd letters")
    odd = {104, 105, 110, 111, 113}
    for j in range(end - start):
        for li, d in enumerate(lengths):
            want = int(start + j + d < end and not (odd & set(range(start + j, start + j + d + 1))))
            assert clean[j, li] == want, (j, d)
    assert 0 < clean.sum() < valid.sum()
    text = mod.deletions_tsv([mod.Region(1, "c", start, end, "odd")], values, encs, clipped, valid, clean, [0, end - start], [dna[start:end]],
                             lengths, 30, "Q")
    lines = text.decode().splitlines()[2:]
    assert len(lines) == int(clean.sum())
    assert all(set(ln.split("\t")[4]) <= set("ACGT") for ln in lines)


# ---- against the existing product on the device ------------------------------------------------------------------------------------
def test_equals_score_variants_on_the_cut_out_context(mod, eng, golden_dir):
    """Every deletion of a 30-position interval with lengths (1, 2, 7), context of 2 030 letters: both alleles' values and encodings
    are those of score_variants for the deletion on the record dna[lo:hi] with flank 2048, whose window is the whole context."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 300)
    dnas = _records(query, p, 91)
    start, end, flank, lengths = 1185, 1215, 1000, (1, 2, 7)
    lo, hi, _, _ = context(dnas[0], start, end, flank)
    assert hi - lo == 2030
    values, encs, _, valid, clean, _ = eng.score_deletions([(0, start, end)], dnas, p, flank=flank, lengths=lengths, queries=[query])
    dels = deletions_of(start, end, lengths)
    assert len(dels) == 29 + 28 + 23 == valid.sum() == clean.sum()
    named = mod.deletion_variants([(0, start, end)], dnas, lengths)
    assert [tuple(t)[2:6] for t in named] == [(start + j, ".", dnas[0][start + j:start + j + lengths[li] + 1].decode(), chr(dnas[0][start + j])) for j, li in dels]
    v, e, _ = eng.score_variants([t._replace(pos=t.pos - lo, rec=0) for t in named], [dnas[0][lo:hi]], p, flank=2048, queries=[query])
    for k, (j, li) in enumerate(dels):
        assert values[0, j, li].tolist() == v[0, k].tolist() and encs[0, j, li].tolist() == e[0, k].tolist(), (j, li)
    assert values.max() > 0 and (values[0, :, :, 0] != values[0, :, :, 1]).any()


# ---- independence -----------------------------------------------------------------------------------------------------------------
def test_independent_of_the_other_intervals_their_order_and_the_engine(mod, golden_dir):
    """Overlapping, nested and repeated intervals on two records, two queries; permuted; one by one; a resident record against a
    passed one.  The engine's own query and a plain scan before and after are untouched, and score_mutagenesis before and after a
    score_deletions call returns identical arrays and counters."""
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
    lengths = (1, 4, 9)
    snv = e.score_mutagenesis(ivs[:3], dnas, p, flank=100, queries=queries)
    snv_stats = {k: v for k, v in e.last_mutagenesis_stats.items() if not k.endswith("_s")}
    values, encs, clipped, valid, clean, offsets = e.score_deletions(ivs, dnas, p, flank=100, lengths=lengths, queries=queries)
    assert values.shape == (2, int(offsets[-1]), 3, 2, 4) and valid.shape == (int(offsets[-1]), 3) and values.max() > 0
    again = e.score_mutagenesis(ivs[:3], dnas, p, flank=100, queries=queries)
    assert all(np.array_equal(a, b) for a, b in zip(snv, again))
    assert snv_stats == {k: v for k, v in e.last_mutagenesis_stats.items() if not k.endswith("_s")}
    perm = [3, 6, 0, 5, 2, 4, 1]
    r2 = e.score_deletions([ivs[k] for k in perm], dnas, p, flank=100, lengths=lengths, queries=queries)
    for at, k in enumerate(perm):
        a, b, a2, b2 = int(offsets[k]), int(offsets[k + 1]), int(r2[5][at]), int(r2[5][at + 1])
        for x, y in zip((values, encs, clipped), r2[:3]):
            assert np.array_equal(y[:, a2:b2], x[:, a:b])
        assert np.array_equal(r2[3][a2:b2], valid[a:b]) and np.array_equal(r2[4][a2:b2], clean[a:b])
    for k, iv in enumerate(ivs):
        a, b = int(offsets[k]), int(offsets[k + 1])
        for q in range(2):
            r1 = e.score_deletions([iv], dnas, p, flank=100, lengths=lengths, queries=[queries[q]])
            assert np.array_equal(r1[0][0], values[q, a:b]) and np.array_equal(r1[1][0], encs[q, a:b]) and np.array_equal(r1[2][0], clipped[q, a:b])
            assert np.array_equal(r1[3], valid[a:b]) and np.array_equal(r1[4], clean[a:b])
    assert np.array_equal(values[:, offsets[0]:offsets[1]], values[:, offsets[4]:offsets[5]])
    e.load_dna(dnas[0])
    res = e.score_deletions([iv for iv in ivs if iv[0] == 0], None, p, flank=100, lengths=lengths, queries=queries)
    keep = np.concatenate([np.arange(offsets[k], offsets[k + 1]) for k, iv in enumerate(ivs) if iv[0] == 0])
    assert np.array_equal(res[0], values[:, keep]) and np.array_equal(res[1], encs[:, keep]) and np.array_equal(res[2], clipped[:, keep])
    assert np.array_equal(res[3], valid[keep]) and np.array_equal(res[4], clean[keep])
    assert e.rna == h19
    after = e.scan(demo, ps)
    assert after.recs == before.recs and after.pool == before.pool
    e.close()


def test_independent_of_the_launches(mod, eng, golden_dir):
    """A 20-nt oligo under 48 encodings and three lengths has 192 problem slots per position, and a launch takes 2^20: two intervals
    of 5 120 and 400 positions (flank 0) are cut into two launches, the cut inside the second interval, whose first range then
    computes the snapshots and own-letter problems of up to 10 positions of the second again; each interval alone is one launch."""
    p = mod.default_params()
    query = _query(golden_dir, 20)
    dna = synth.random_dna(5600, 95)
    ivs = [(0, 0, 5120), (0, 5100, 5500)]
    lengths = (1, 3, 10)
    values, encs, clipped, valid, clean, offsets = eng.score_deletions(ivs, [dna], p, flank=0, lengths=lengths, queries=[query])
    assert eng.last_deletion_stats["launches"] == 2 and eng.last_deletion_stats["prefix_problems"] == 3 * 48
    for k, iv in enumerate(ivs):
        a, b = int(offsets[k]), int(offsets[k + 1])
        r1 = eng.score_deletions([iv], [dna], p, flank=0, lengths=lengths, queries=[query])
        assert eng.last_deletion_stats["launches"] == 1
        assert np.array_equal(r1[0][0], values[0, a:b]) and np.array_equal(r1[1][0], encs[0, a:b]) and np.array_equal(r1[2][0], clipped[0, a:b])
        assert np.array_equal(r1[3], valid[a:b]) and np.array_equal(r1[4], clean[a:b])
    assert values.max() > 0 and valid.sum() == sum(max(0, e - s - d) for _, s, e in ivs for d in lengths)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(mod, eng, golden_dir):
    rec = synth.random_dna(6000, 3)
    q = _query(golden_dir, 30)
    p = mod.default_params(rule=1)
    cases = [
        (dict(lengths=()), mod.E_ARG),
        (dict(lengths=tuple(range(1, 18))), mod.E_ARG),                     # 17 lengths
        (dict(lengths=(2, 1)), mod.E_ARG),
        (dict(lengths=(3, 3)), mod.E_ARG),
        (dict(lengths=(0,)), mod.E_ARG),
        (dict(lengths=(1, 1024)), mod.E_ARG),
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
        # one position alone does not fit a launch: 48 encodings x 497 snapshot columns x 4 bytes x 2 816 rows > 256 MB
        (dict(queries=[_query(golden_dir, 2812)], p=mod.default_params(), intervals=[(0, 0, 600)], lengths=(1, 496)), mod.E_UNSUPPORTED),
    ]
    for kw, code in cases:
        args = dict(intervals=[(0, 50, 56)], dnas=[rec], p=p, flank=20, lengths=(1, 2), queries=[q])
        args.update(kw)
        with pytest.raises(mod.FasimError) as ei:
            eng.score_deletions(**args)
        assert ei.value.code == code, (kw.keys(), str(ei.value))
    _check(eng, q, [rec], [(0, 50, 56)], 20, (1, 2), p, "after the refusals")
    eng.score_deletions([(0, 0, 5080)], [rec], p, flank=20, lengths=tuple(range(1, 17)), queries=[q[:4]])      # the widest context, 16 lengths
    # the longest length that H19's 2 816 rows take under 48 encodings, and a longer one in an interval too short to reach it
    eng.score_deletions([(0, 0, 497)], [rec], mod.default_params(), flank=0, lengths=(495,), queries=[_query(golden_dir, 2812)])
    eng.score_deletions([(0, 0, 300)], [rec], mod.default_params(), flank=0, lengths=(1, 900), queries=[_query(golden_dir, 2812)])


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_tables(mod, eng, tmp_path, golden_dir):
    """The deletions table equals deletions_tsv of the Python results byte for byte; the mutagenesis table is the same with and
    without --deletions; --deletions-only writes one file; an interval that no record holds gives status 1."""
    q = _query(golden_dir, 60)
    p = mod.default_params()
    dnas = _records(q, p, 41)
    chr1, chr2 = dnas
    chr1 = chr1[:995] + b"n" + chr1[996:]                                  # deletions without lines
    dnas = [chr1, chr2]
    synth.write_fasta(str(tmp_path / "g.fa"), "chr1 test record", chr1)
    with open(tmp_path / "g.fa", "a") as f:
        f.write(">chr2\n" + chr2.decode() + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + q.decode() + "\n")
    good = ["chr1\t990\t1010\tsite\n", "chr2\t495\t500\n", "chr1\t1195\t1205\tsite\n"]
    bad = ["chr7\t10\t20\tlost\n", "chr2\t495\t501\tpast\n"]
    lengths = (1, 2, 5)
    runs = (("all.bed", ["# intervals\n", good[0], bad[0], good[1], bad[1], good[2]], 1, ("--deletions", "1,2,5"), ["Q-g.deletions.tsv", "Q-g.mutagenesis.tsv"]),
            ("good.bed", good, 0, ("--deletions", "1,2,5"), ["Q-g.deletions.tsv", "Q-g.mutagenesis.tsv"]),
            ("plain.bed", good, 0, (), ["Q-g.mutagenesis.tsv"]),
            ("only.bed", good, 0, ("--deletions", "1,2,5", "--deletions-only"), ["Q-g.deletions.tsv"]))
    tables = {}
    for name, lines, status, extra, files in runs:
        (tmp_path / name).write_text("".join(lines))
        out = tmp_path / ("out_" + name)
        out.mkdir()
        r = subprocess.run([EXE, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--mutagenesis", name, "--mutagenesis-flank", "150", *extra],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == status, r.stderr
        assert sorted(os.listdir(out)) == files
        tables[name] = {f: (out / f).read_bytes() for f in files}
        if "Q-g.deletions.tsv" not in files:
            continue
        regions = mod.read_bed(str(tmp_path / name))
        held = [g for g in regions if g.name not in ("lost", "past")]
        ivs = [(1 if g.chrom == "chr2" else 0, g.start, g.end) for g in held]
        values, encs, clipped, valid, clean, offsets = eng.score_deletions(ivs, dnas, p, flank=150, lengths=lengths, queries=[q])
        full, seqs, at = [0], [], 0
        for g in regions:
            if g in held:
                seqs.append(dnas[ivs[at][0]][g.start:g.end])
                at += 1
            else:
                seqs.append(None)
            full.append(int(offsets[at]))
        want = mod.deletions_tsv(regions, values[0], encs[0], clipped[0], valid, clean, full, seqs, lengths, 150, "Q")
        got = tables[name]["Q-g.deletions.tsv"]
        assert got == want
        assert got.startswith(b"# fasim deletions lncRNA=Q flank=150 lengths=1,2,5\nline\tchrom\tpos\tid\tref\talt\t")
        assert got.count(b"\n") == 2 + int(clean.sum()) and clean.sum() == valid.sum() - 2 - 3 - 6 and b"\tsite_" in got
        if status:
            for word in ("BED line 3 (lost) chr7:10-20: no DNA record of its chromosome", "BED line 5 (past)", "runs past the end", "2 of 5 BED intervals"):
                assert word in r.stderr, r.stderr
        else:
            assert "finished normally" in r.stdout
    assert tables["good.bed"]["Q-g.mutagenesis.tsv"] == tables["plain.bed"]["Q-g.mutagenesis.tsv"]
    assert tables["good.bed"]["Q-g.deletions.tsv"] == tables["only.bed"]["Q-g.deletions.tsv"]
