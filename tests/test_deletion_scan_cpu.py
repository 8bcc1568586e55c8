"""Every deletion of an interval from the shared pass (fasim_score_deletions), the part that needs no GPU: the
yardstick of the GPU tests, expected_deletions, built on the restatement of section 19 (test_variants_cpu.touch_units) exactly as the
definition reads -- one context per interval, one REF and one ALT unit per (deletion, encoding) -- and tied to the old yardstick
expected_scores on the cut-out context; jump_life, a numpy restatement of the shared pass (snapshots, column maxima, jump problems)
that is held to expected_deletions word for word and also says how many columns the jump problems run; and the pure host functions
deletions_tsv and deletion_variants, the exported symbols and the CLI's usage errors.

Neither restatement calls the code under test."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_mutagenesis_cpu import _planted, context
from test_track_cpu import _CODE, enabled_encodings, enc_class, encode_unit
from test_variants_cpu import CLASS_NAMES, expected_scores, touch_units

ACGT = b"ACGT"


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


# ---- the definition: what Engine.score_deletions must return -------------------------------------------------------------------------
def deletions_of(start: int, end: int, lengths):
    """The (position offset, length index) pairs that are deletions: x + d < end."""
    return [(x - start, li) for x in range(start, end) for li, d in enumerate(lengths) if x + d < end]


def fold(words, npos: int, lengths, encs):
    """values (npos, nlen, 2, 4), encs (npos, nlen, 2, 4), clipped (npos, nlen, 2) from the words {(j, li, allele, enc): 2 * value +
    bit}: per class the largest value and the smallest encoding that attains it, the bit of the allele's largest word."""
    nlen = len(lengths)
    values = np.zeros((npos, nlen, 2, 4), dtype=np.int64)
    which = np.full((npos, nlen, 2, 4), -1, dtype=np.int64)
    clipped = np.zeros((npos, nlen, 2), dtype=np.int64)
    for (j, li) in sorted({(j, li) for j, li, _, _ in words}):
        for al in range(2):
            top = 0
            for c in range(4):
                mine = [(words[(j, li, al, e)], e) for e in encs if enc_class(e) == c]
                if not mine:
                    continue
                big = max(w for w, _ in mine)
                top = max(top, big)
                values[j, li, al, c] = big >> 1
                if big >> 1:
                    which[j, li, al, c] = min(e for w, e in mine if w >> 1 == big >> 1)
            clipped[j, li, al] = top & 1
    return values, which, clipped


def expected_words(rna: bytes, dna: bytes, start: int, end: int, flank: int, lengths, p):
    """{(j, li, allele, enc): 2 * value + bit} of the definition: REF the context with the mark [c0, c0 + d + 1), ALT the context
    without the letters [c0 + 1, c0 + 1 + d) with the mark [c0, c0 + 1), both with the context's edges; an odd encoding's target is
    reversed, its mark mirrored in the unit's own length and its edges swapped."""
    encs = enabled_encodings(p)
    lo, hi, e_lo, e_hi = context(dna, start, end, flank)
    C = dna[lo:hi]
    n = len(C)
    words = {}
    for li, d in enumerate(lengths):      # ALT units of one length have one width
        for al in range(2):
            units, keys = [], []
            for x in range(start, end):
                if x + d >= end:
                    continue
                c0 = x - lo
                w, v0, v1 = (C, c0, c0 + d + 1) if al == 0 else (C[:c0 + 1] + C[c0 + 1 + d:], c0, c0 + 1)
                nw = len(w)
                for e in encs:
                    units.append((encode_unit(w, e), nw - v1, nw - v0, e_hi, e_lo) if e & 1 else (encode_unit(w, e), v0, v1, e_lo, e_hi))
                    keys.append((x - start, li, al, e))
            if units:
                got = touch_units(rna, [u[0] for u in units], [u[1] for u in units], [u[2] for u in units], [u[3] for u in units], [u[4] for u in units])
                words.update({k: int(g) for k, g in zip(keys, got)})
    return words


def expected_deletions(rna: bytes, dna: bytes, start: int, end: int, flank: int, lengths, p):
    """values (L, nlen, 2, 4), encs (L, nlen, 2, 4), clipped (L, nlen, 2), valid (L, nlen), clean (L, nlen) of the definition for
    one query and one interval."""
    L, nlen = end - start, len(lengths)
    values, which, clipped = fold(expected_words(rna, dna, start, end, flank, lengths, p), L, lengths, enabled_encodings(p))
    valid = np.zeros((L, nlen), dtype=np.int64)
    clean = np.zeros((L, nlen), dtype=np.int64)
    for j, li in deletions_of(start, end, lengths):
        valid[j, li] = 1
        clean[j, li] = all(c in ACGT for c in dna[start + j:start + j + lengths[li] + 1])
    return values, which, clipped, valid, clean


# ---- the shared pass, restated ---------------------------------------------------------------------------------------------------------
def _floor(x):
    return np.where(x >= 2, x, 0)


def _column(H, E, t, cont, cut, score, down):
    """One column of the touching matrix for several problems at once: H, E (problems, m) of the previous column in doubled values,
    t the column's code, cont whether the diagonal only continues, cut whether the column carries the clip bit (all per problem).
    Returns H and E of the column."""
    E = _floor(np.maximum(E - 8, H - 32))
    d = np.concatenate([np.zeros((H.shape[0], 1), dtype=np.int64), H[:, :-1]], axis=1)
    dg = d + score[t]
    dg = np.where(cont[:, None] & (d == 0), 0, dg)
    h = _floor(np.maximum(dg, E))
    h = np.where(cut[:, None] & (h > 0), h | 1, h)
    reach = np.maximum.accumulate(h + down, axis=1)
    F = np.zeros_like(h)
    F[:, 1:] = _floor(reach[:, :-1] - down[1:] - 24)
    H = np.maximum(h, F)
    H = np.where(cut[:, None] & (H > 0), H | 1, H)
    return H, E


def jump_life(rna: bytes, dna: bytes, start: int, end: int, flank: int, lengths, p):
    """The shared pass of section 27 for one query and one interval taken as one group: per encoding the plain recurrence over the
    context's (mirrored) codes with the row state S[j] before every column and the column maxima pm[j]; the own-letter jump problems
    (y, y, y + 1) of the columns that are the last of a REF mark; the ALT jump problems; REF = max(pm over the first d mark columns,
    own of the last).  Returns ({(j, li, allele, enc): word}, info) with info's own_problems, alt_problems, cont_cols (the columns the jump
    problems ran until their dead column) and cont_cols_bound (the sum of 1 + n - r)."""
    encs = enabled_encodings(p)
    lo, hi, e_lo, e_hi = context(dna, start, end, flank)
    C = dna[lo:hi]
    n, ne = len(C), len(encs)
    dels = deletions_of(start, end, lengths)
    info = dict(own_problems=0, alt_problems=0, cont_cols=0, cont_cols_bound=0)
    if not dels or not ne:
        return {}, info
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    m = len(q)
    score = np.where((q[None, :] == np.arange(5)[:, None]) & (q[None, :] < 4), 10, -8)
    down = 8 * np.arange(m, dtype=np.int64)
    tc = np.stack([_CODE[np.frombuffer(encode_unit(C, e), dtype=np.uint8)] for e in encs])      # (ne, n), mirrored for odd e
    odd = np.array([e & 1 for e in encs], dtype=bool)
    first_cut = np.where(odd, e_hi, e_lo)      # the unit's first / last column is a cut end
    last_cut = np.where(odd, e_lo, e_hi)
    # the prefix pass: snapshots and column maxima
    SH = np.zeros((n, ne, m), dtype=np.int64)
    SE = np.zeros((n, ne, m), dtype=np.int64)
    pm = np.zeros((n, ne), dtype=np.int64)
    H = np.zeros((ne, m), dtype=np.int64)
    E = np.zeros((ne, m), dtype=np.int64)
    never = np.zeros(ne, dtype=bool)
    for j in range(n):
        SH[j], SE[j] = H, E
        H, E = _column(H, E, tc[:, j], never, first_cut if j == 0 else never, score, down)      # (column n - 1 is never read from pm)
        pm[j] = H.max(axis=1)
    # the jump problems (encoding index, s, k, r): own-letter ones once per (column, encoding), ALT ones per (deletion, encoding)
    probs, keys = [], []
    for k, e in enumerate(encs):
        # the last mark column of REF: where a deletion ends or, mirrored, where one is anchored
        for y in sorted({start + j + (0 if e & 1 else lengths[li]) - lo for j, li in dels}):
            a = n - 1 - y if e & 1 else y
            probs.append((k, a, a, a + 1))
            keys.append(("own", y, e))
        for j, li in dels:
            c0, d = start + j - lo, lengths[li]
            a = n - 1 - c0 if e & 1 else c0
            probs.append((k, a - d, a, a + 1) if e & 1 else (k, a, a, a + 1 + d))
            keys.append(("alt", j, li, e))
    pk, ps, pc, pr = (np.array(v, dtype=np.int64) for v in zip(*probs))
    np_ = len(probs)
    H, E = SH[ps, pk].copy(), SE[ps, pk].copy()
    best = np.zeros(np_, dtype=np.int64)
    ran = np.zeros(np_, dtype=np.int64)
    alive = np.ones(np_, dtype=bool)
    col = pc.copy()
    for step in range(n):
        alive &= col < n
        if not alive.any():
            break
        c = np.minimum(col, n - 1)
        if step == 0:
            cut = ((ps == 0) & first_cut[pk]) | ((pr == n) & last_cut[pk])
        else:
            cut = (c == n - 1) & last_cut[pk]
        H2, E2 = _column(H, E, tc[pk, c], np.full(np_, step > 0), cut, score, down)
        H = np.where(alive[:, None], H2, H)
        E = np.where(alive[:, None], E2, E)
        best = np.where(alive, np.maximum(best, H.max(axis=1)), best)
        ran += alive
        alive &= H.any(axis=1) | E.any(axis=1)      # a dead column: every later one is dead
        col = np.where(step == 0, pr, col + 1)
    got = {k: (int(b), int(r)) for k, b, r in zip(keys, best, ran)}
    info["own_problems"] = sum(1 for k in keys if k[0] == "own")
    info["alt_problems"] = sum(1 for k in keys if k[0] == "alt")
    info["cont_cols"] = int(ran.sum())
    info["cont_cols_bound"] = int((1 + n - pr).sum())
    words = {}
    for k, e in enumerate(encs):
        for j, li in dels:
            c0, d = start + j - lo, lengths[li]
            if e & 1:
                a = n - 1 - c0
                ref = max(int(pm[a - d:a, k].max()), got[("own", c0, e)][0])
            else:
                ref = max(int(pm[c0:c0 + d, k].max()), got[("own", c0 + d, e)][0])
            words[(j, li, 0, e)] = ref
            words[(j, li, 1, e)] = got[("alt", j, li, e)][0]
    return words, info


def early_stop_case():
    """A 20-nt oligo on random DNA, flank 300, 8 positions, lengths (1, 5): (query, dna, (rec, start, end), flank, lengths)."""
    return synth.random_rna(20, 271), synth.random_dna(2000, 272), (0, 1000, 1008), 300, (1, 5)


# ---- the restatements against each other -----------------------------------------------------------------------------------------------
def test_jump_life_equals_the_definition_word_for_word():
    """Random and planted records, query lengths 1 to 113, even and odd encodings, every combination of cut ends (flank and interval
    chosen so that the context is cut at neither, either or both ends), deletions that end at the context's last column."""
    m = _mod()
    n = 0
    for k, mq in enumerate((1, 7, 20, 40, 113)):
        p = m.default_params(rule=1 + k % 3)
        for rep, (start, end, flank) in enumerate(((55, 66, 30), (0, 6, 10), (150, 160, 25), (57, 64, 0), (0, 160, 0), (3, 12, 2))):
            rna, dna = _planted(mq, 700 + 10 * k + rep) if rep % 2 == 0 else (synth.random_rna(mq, 40 + k), synth.random_dna(160, 50 + rep))
            lengths = ((1, 2, 5), (1, 4), (3,), (1, 2, 3, 6), (1, 60), (2, 8))[rep]
            want = expected_words(rna, dna, start, end, flank, lengths, p)
            got, info = jump_life(rna, dna, start, end, flank, lengths, p)
            assert got == want, (mq, rep)
            assert len(want) == 2 * len(enabled_encodings(p)) * len(deletions_of(start, end, lengths))
            assert 0 < info["cont_cols"] <= info["cont_cols_bound"]
            assert {e & 1 for e in enabled_encodings(p)} == {0, 1}
            n += len(want) // 2
    assert n > 2000


def test_definition_ties_to_the_old_yardstick_on_the_cut_out_context():
    """For every deletion of four intervals the values and encodings are those of expected_scores for the same deletion on the
    record dna[lo:hi] with a flank that covers it.  (Flags are not compared: a cut-out record's ends are record ends.)  Also: a
    value is never below the value of the deletion's own, smaller window."""
    m = _mod()
    p = m.default_params(rule=1)
    lengths = (1, 2, 5)
    for seed, (start, end, flank) in enumerate(((55, 66, 30), (0, 6, 10), (150, 160, 25), (57, 64, 0))):
        rna, dna = _planted(40, 900 + seed)
        values, which, clipped, valid, clean = expected_deletions(rna, dna, start, end, flank, lengths, p)
        lo, hi, _, _ = context(dna, start, end, flank)
        dels = deletions_of(start, end, lengths)
        assert valid.sum() == len(dels) > 0 and (clean == valid).all()
        V = [m.Variant(1, "c", start + j - lo, ".", dna[start + j:start + j + lengths[li] + 1].decode(), chr(dna[start + j])) for j, li in dels]
        ev, ew, _ = expected_scores(rna, [dna[lo:hi]], V, hi - lo, p)
        own, _, _ = expected_scores(rna, [dna], [v._replace(pos=v.pos + lo) for v in V], flank, p)
        for k, (j, li) in enumerate(dels):
            assert values[j, li].tolist() == ev[k].tolist() and which[j, li].tolist() == ew[k].tolist(), (seed, j, li)
            assert (values[j, li] >= own[k]).all()
        assert values.max() > 0
        assert not values[valid == 0].any() and (which[valid == 0] == -1).all()


def test_the_early_stop_holds_for_the_gpu_tests_input():
    """The condition test_gpu_deletion_scan asserts on the engine's counters, known to hold for the input before any GPU run."""
    m = _mod()
    rna, dna, (_, start, end), flank, lengths = early_stop_case()
    words, info = jump_life(rna, dna, start, end, flank, lengths, m.default_params())
    assert len(enabled_encodings(m.default_params())) == 48
    assert info["cont_cols"] * 2 < info["cont_cols_bound"], info
    assert info["alt_problems"] == 48 * (8 - 1 + 8 - 5) and info["own_problems"] == 48 * 7


# ---- the surface -------------------------------------------------------------------------------------------------------------------------
def test_deletion_symbols_are_exported():
    m = _mod()
    for s in ("fasim_score_deletions", "fasim_deletions_tsv"):
        assert s in m.EXPORTS and hasattr(m.lib(), s)
    for name in ("deletions_tsv", "deletion_variants"):
        assert callable(getattr(m, name))
    assert callable(m.Engine.score_deletions) and m.MAX_DELETION_LENGTHS == 16
    hdr = open(os.path.join(entry.ROOT, "include", "fasim_hip.h")).read()
    for word in ("FASIM_MAX_DELETION_LENGTHS 16", "fasim_del_score", "fasim_deletion_stats", "fasim_score_deletions", "fasim_deletions_tsv"):
        assert word in hdr


HEAD = "line\tchrom\tpos\tid\tref\talt" + "".join(f"\t{c}_ref\t{c}_alt" for c in CLASS_NAMES) + "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n"


def test_deletions_tsv_bytes():
    """Three positions of one interval under lengths (1, 2) and an interval that was not scored: the pairs that are no deletions and
    the unclean one get no lines; a value of 0 prints NA for its rule; the clip flag is the bit of the larger of the two alleles'
    words, and a tie goes to the bit."""
    m = _mod()
    regions = [m.Region(4, "chr1", 99, 102, "site"), m.Region(6, "chr2", 5, 9, "lost")]
    values = np.zeros((3, 2, 2, 4), dtype=np.int32)
    encs = np.full((3, 2, 2, 4), -1, dtype=np.int8)
    clipped = np.zeros((3, 2, 2), dtype=np.uint8)
    valid = np.array([[1, 1], [1, 0], [0, 0]], dtype=np.uint8)
    clean = np.array([[1, 0], [1, 0], [0, 0]], dtype=np.uint8)      # (0, 2) is marked unclean
    values[0, 0, 0] = [50, 0, 75, 60]; encs[0, 0, 0] = [2, -1, 16, 13]         # REF: max 75, enc 16 -> rule 3
    values[0, 0, 1] = [41, 0, 84, 60]; encs[0, 0, 1] = [2, -1, 18, 47]         # ALT: max 84, enc 18 -> rule 4
    values[0, 1] = 999                                                         # unclean: never printed
    values[1, 0, 0] = [0, 20, 75, 0]; encs[1, 0, 0] = [-1, 11, 14, -1]         # REF 75 unclipped, ALT 75 clipped: a tie, the bit wins
    values[1, 0, 1] = [75, 0, 0, 0]; encs[1, 0, 1] = [0, -1, -1, -1]
    clipped[1, 0, 1] = 1
    values[1, 1] = 7                                                           # no deletion: never printed
    got = m.deletions_tsv(regions, values, encs, clipped, valid, clean, [0, 3, 3], [b"GAC", None], (1, 2), 300, "MEG3")
    want = ("# fasim deletions lncRNA=MEG3 flank=300 lengths=1,2\n" + HEAD +
            "4\tchr1\t100\tsite\tGA\tG\t50\t41\t0\t0\t75\t84\t60\t60\t75\t84\t9\t3\t4\t0\n"
            "4\tchr1\t101\tsite\tAC\tA\t0\t75\t20\t0\t75\t0\t0\t0\t75\t75\t0\t2\t1\t1\n")
    assert got == want.encode()
    clean[1, 0] = 0
    clean[0, 0] = 0
    assert m.deletions_tsv(regions, values, encs, clipped, valid, clean, [0, 3, 3], [b"GAC", None], (1, 2), 300, "MEG3") == \
        ("# fasim deletions lncRNA=MEG3 flank=300 lengths=1,2\n" + HEAD).encode()
    assert m.deletions_tsv([], np.zeros((0, 1, 2, 4)), np.zeros((0, 1, 2, 4)), np.zeros((0, 1, 2)), np.zeros((0, 1)), np.zeros((0, 1)), [0], [],
                           (7,), 0, "q") == ("# fasim deletions lncRNA=q flank=0 lengths=7\n" + HEAD).encode()
    for bad in ((), (2, 2), (0,), (1024,), tuple(range(1, 18))):
        with pytest.raises(m.FasimError) as ei:
            m.deletions_tsv([], np.zeros((0, len(bad), 2, 4)), np.zeros((0, len(bad), 2, 4)), np.zeros((0, len(bad), 2)), np.zeros((0, len(bad))),
                            np.zeros((0, len(bad))), [0], [], bad, 0, "q")
        assert ei.value.code == m.E_ARG


def test_deletion_variants_names_the_clean_deletions_in_table_order():
    m = _mod()
    dnas = [b"ACNgTAC", b"GGT"]
    got = m.deletion_variants([(0, 0, 7), (1, 0, 3), (1, 2, 3)], dnas, (1, 2))
    assert [tuple(v) for v in got] == [
        (1, "rec0", 0, ".", "AC", "A", 0, True), (1, "rec0", 4, ".", "TA", "T", 0, True), (1, "rec0", 4, ".", "TAC", "T", 0, True),
        (1, "rec0", 5, ".", "AC", "A", 0, True),
        (2, "rec1", 0, ".", "GG", "G", 1, True), (2, "rec1", 0, ".", "GGT", "G", 1, True), (2, "rec1", 1, ".", "GT", "G", 1, True)]
    assert m.deletion_variants([], dnas, (1,)) == []


# ---- the CLI: usage errors exit 2 before any engine exists and write nothing ---------------------------------------------------------
def _cli(tmp_path, *args):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    (tmp_path / "m.bed").write_text("chr1\t10\t40\tsite\n")
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    return r, sorted(os.listdir(out))


@pytest.mark.parametrize("args", [("--deletions", "1,2"), ("--deletions-only",), ("--deletions", "1", "--deletions-only")], ids=["list", "only", "both"])
def test_cli_deletions_need_mutagenesis(tmp_path, args):
    r, written = _cli(tmp_path, *args)
    assert r.returncode == 2 and "--mutagenesis" in r.stderr, r.stderr
    assert written == []


def test_cli_deletions_only_needs_a_list(tmp_path):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", "--deletions-only")
    assert r.returncode == 2 and "--deletions" in r.stderr, r.stderr
    assert written == []


@pytest.mark.parametrize("text", ["", "2,1", "1,1", "1,x", "1.5", "0", "1024", "-1", "1,", ",1", "1,,2", ",".join(str(d) for d in range(1, 18))],
                         ids=["empty", "unsorted", "repeated", "letter", "fraction", "zero", "1024", "negative", "trailing", "leading", "hole", "17"])
def test_cli_bad_deletion_list_exits_2(tmp_path, text):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", "--deletions", text)
    assert r.returncode == 2 and "--deletions" in r.stderr, r.stderr
    assert written == []
