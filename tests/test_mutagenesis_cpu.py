"""Every SNV of an interval from one shared pass (fasim_score_mutagenesis), the part that needs no GPU: the
yardstick of the GPU tests, expected_mutagenesis, built on the restatement of section 19 (test_variants_cpu.touch_units) exactly as
the definition reads -- one context per interval, one byte exchanged, the mark on that byte -- and tied to the old yardstick
expected_scores on the cut-out context; touch_life, a restatement of one problem that also says how many columns it runs until its
dead column, held to touch_units; and the pure host functions mutagenesis_tsv and mutagenesis_variants, and the CLI's usage errors.

Neither restatement calls the code under test."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, enabled_encodings, enc_class, encode_unit
from test_variants_cpu import CLASS_NAMES, expected_scores, touch_units

ACGT = b"ACGT"


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(autouse=True)
def _feature():
    """Without the product's symbols none of these tests has anything to measure."""
    m = _mod()
    assert "fasim_score_mutagenesis" in m.EXPORTS and hasattr(m.lib(), "fasim_score_mutagenesis")


# ---- one problem, with its life ------------------------------------------------------------------------------------------------------
def touch_life(rna: bytes, targets, col, edge_lo, edge_hi):
    """(2 * value + b, columns run) of several units of one length whose mark is the single column col (one per unit or a scalar):
    E[i][j] = floor(max(E[i][j-1] - 8, H[i][j-1] - 32)), F likewise down the column, H = floor(max(diagonal, E)) then max with F, in
    doubled values; the diagonal is H[i-1][j-1] + 2 s up to column col and only continues a positive H[i-1][j-1] behind it.  The
    value is the maximum of H over the columns from col on.  The columns run: from col up to and including the first column in which
    every H and E is zero -- behind it nothing can be above zero -- or up to the last column."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = np.stack([_CODE[np.frombuffer(x, dtype=np.uint8)] for x in targets])
    nu, n = t.shape
    m = len(q)
    col = np.broadcast_to(np.asarray(col, dtype=np.int64), (nu,))
    edge_lo = np.broadcast_to(np.asarray(edge_lo, dtype=bool), (nu,))
    edge_hi = np.broadcast_to(np.asarray(edge_hi, dtype=bool), (nu,))
    score = np.where((q[None, :] == np.arange(5)[:, None]) & (q[None, :] < 4), 10, -8)        # (5, m)
    down = 8 * np.arange(m, dtype=np.int64)
    H = np.zeros((nu, m), dtype=np.int64)
    E = np.zeros((nu, m), dtype=np.int64)
    best = np.zeros(nu, dtype=np.int64)
    ran = n - col
    alive = np.ones(nu, dtype=bool)

    def floor(x):
        return np.where(x >= 2, x, 0)
    for j in range(n):
        E = floor(np.maximum(E - 8, H - 32))
        d = np.concatenate([np.zeros((nu, 1), dtype=np.int64), H[:, :-1]], axis=1)
        dg = d + score[t[:, j]]
        dg = np.where((j > col)[:, None] & (d == 0), 0, dg)
        cut = (((j == 0) & edge_lo) | ((j == n - 1) & edge_hi))[:, None]
        h = floor(np.maximum(dg, E))
        h = np.where(cut & (h > 0), h | 1, h)
        # F[i] = floor(max over k < i of (h[k] - 32 - 8 (i - 1 - k)))
        reach = np.maximum.accumulate(h + down, axis=1)
        F = np.zeros_like(h)
        F[:, 1:] = floor(reach[:, :-1] - down[1:] - 24)
        H = np.maximum(h, F)
        H = np.where(cut & (H > 0), H | 1, H)
        best = np.where(j >= col, np.maximum(best, H.max(axis=1)), best)
        dead = alive & (j >= col) & ~(H.any(axis=1) | E.any(axis=1))
        ran = np.where(dead, j - col + 1, ran)
        alive &= ~dead
    return best, ran


# ---- the whole definition: what Engine.score_mutagenesis must return ----------------------------------------------------------------
def context(dna: bytes, start: int, end: int, flank: int):
    lo, hi = max(0, start - flank), min(len(dna), end + flank)
    return lo, hi, lo > 0, hi < len(dna)


def expected_mutagenesis(rna: bytes, dna: bytes, start: int, end: int, flank: int, p, life: bool = True):
    """values (L, 4, 4), encs (L, 4, 4), ref (L,), clipped (L, 4) of the definition for one query and one interval, and a dict with
    cont_cols (touch_life's columns over all problems; None without `life`) and cont_cols_bound."""
    encs = enabled_encodings(p)
    lo, hi, e_lo, e_hi = context(dna, start, end, flank)
    C = dna[lo:hi]
    n, L = len(C), end - start
    units, keys = [], []
    for x in range(start, end):
        for b in range(4):
            w = C[:x - lo] + ACGT[b:b + 1] + C[x - lo + 1:]
            v0 = x - lo
            for e in encs:
                units.append((encode_unit(w, e), n - v0 - 1, n - v0, e_hi, e_lo) if e & 1 else (encode_unit(w, e), v0, v0 + 1, e_lo, e_hi))
                keys.append((x - start, b, e))
    words = np.zeros(0, dtype=np.int64)
    cont = None
    if units:
        words = touch_units(rna, [u[0] for u in units], [u[1] for u in units], [u[2] for u in units], [u[3] for u in units], [u[4] for u in units])
        if life:
            lw, ran = touch_life(rna, [u[0] for u in units], [u[1] for u in units], [u[3] for u in units], [u[4] for u in units])
            assert lw.tolist() == words.tolist()
            cont = int(ran.sum())
    got = {k: int(w) for k, w in zip(keys, words)}
    values = np.zeros((L, 4, 4), dtype=np.int64)
    which = np.full((L, 4, 4), -1, dtype=np.int64)
    clipped = np.zeros((L, 4), dtype=np.int64)
    ref = np.array([ACGT.find(dna[x:x + 1]) for x in range(start, end)], dtype=np.int64)
    for j in range(L):
        for b in range(4):
            top = 0
            for c in range(4):
                mine = [(got[(j, b, e)], e) for e in encs if enc_class(e) == c]
                if not mine:
                    continue
                big = max(w for w, _ in mine)
                top = max(top, big)
                values[j, b, c] = big >> 1
                if big >> 1:
                    which[j, b, c] = min(e for w, e in mine if w >> 1 == big >> 1)
            clipped[j, b] = top & 1
    bound = sum(n - u[1] for u in units)
    return values, which, ref, clipped, dict(cont_cols=cont, cont_cols_bound=bound)


def _planted(m: int, seed: int):
    """(rna, dna): 160 nt of random DNA with a gapped copy of a stretch of the query's encoding-0 pre-image across column 60."""
    rna = synth.random_rna(m, seed)
    dna = bytearray(synth.random_dna(160, seed + 1))
    piece = rna[:min(m, 30)].replace(b"U", b"A")
    pre = bytearray(piece.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A").replace(b"C", b"T"))      # encoding 0: A T G C -> T G G T
    if len(pre) > 12:
        del pre[len(pre) // 2]
    dna[60 - len(pre) // 2:60 - len(pre) // 2 + len(pre)] = pre
    return rna, bytes(dna[:160])


def test_touch_life_equals_touch_units_and_stops_early():
    """Value and bit over random and planted targets, every combination of cut ends, marks at the first, the last and inner
    columns; the columns run lie in [1, n - col], reach n - col where an alignment runs to the last column, and are fewer than that
    in most random cases."""
    short = total = 0
    for k, m in enumerate((1, 7, 20, 40, 113)):
        for rep in range(24):
            seed = 500 + 40 * k + rep
            rna, dna = _planted(m, seed) if rep % 2 else (synth.random_rna(m, seed), synth.random_dna(90 + rep, seed + 7))
            n = len(dna)
            cols = [0, n - 1, n // 3, 60 if n > 60 else n // 2]
            tg = [encode_unit(dna, 0)] * len(cols)
            lo, hi = bool(rep & 1), bool(rep & 2)
            words, ran = touch_life(rna, tg, cols, lo, hi)
            want = touch_units(rna, tg, cols, [c + 1 for c in cols], lo, hi)
            assert words.tolist() == want.tolist(), (m, rep)
            for c, r in zip(cols, ran.tolist()):
                assert 1 <= r <= n - c
                total += 1
                short += r < n - c
    assert short * 2 > total, (short, total)
    # a perfect copy that runs from the mark to the last column keeps the problem alive to the end and, cut there, carries the bit
    rna = b"AGGAGAAGGAGAGGAAGAGA"
    tgt = b"CCCCCCCCCC" + rna
    w, r = touch_life(rna, [tgt], 12, False, True)
    assert (int(w[0]), int(r[0])) == (2 * 100 + 1, len(tgt) - 12)
    w, r = touch_life(rna, [tgt + b"C" * 40], 12, False, True)
    assert int(w[0]) == 2 * 100 and int(r[0]) < len(tgt) + 40 - 12


def test_definition_ties_to_the_old_yardstick_on_the_cut_out_context():
    """For every SNV of an interval the values and encodings are those of expected_scores for the same SNV on the record dna[lo:hi]
    with a flank of hi - lo: there the variant's own window is the whole context.  (Flags are not compared: a cut-out record's ends
    are record ends.)  Also: a value here is never below the value of the SNV's own, smaller window."""
    m = _mod()
    p = m.default_params(rule=1)
    for seed, (start, end, flank) in enumerate(((55, 63, 30), (0, 5, 10), (150, 160, 25), (58, 60, 0))):
        rna, dna = _planted(40, 900 + seed)
        values, which, ref, clipped, info = expected_mutagenesis(rna, dna, start, end, flank, p)
        lo, hi, _, _ = context(dna, start, end, flank)
        assert info["cont_cols"] <= info["cont_cols_bound"]
        snvs = [(x, b) for x in range(start, end) for b in range(4)]
        V = [m.Variant(1, "c", x - lo, ".", chr(dna[x]), chr(ACGT[b])) for x, b in snvs]
        ev, ew, _ = expected_scores(rna, [dna[lo:hi]], V, hi - lo, p)
        own, _, _ = expected_scores(rna, [dna], [m.Variant(1, "c", x, ".", chr(dna[x]), chr(ACGT[b])) for x, b in snvs], flank, p)
        for k, (x, b) in enumerate(snvs):
            r = int(ref[x - start])
            assert r == ACGT.find(dna[x:x + 1]) and r >= 0
            assert values[x - start, b].tolist() == ev[k, 1].tolist() and which[x - start, b].tolist() == ew[k, 1].tolist()
            assert values[x - start, r].tolist() == ev[k, 0].tolist() and which[x - start, r].tolist() == ew[k, 0].tolist()
            assert (values[x - start, b] >= own[k, 1]).all() and (values[x - start, r] >= own[k, 0]).all()
        assert values.max() > 0


def test_mutagenesis_symbols_are_exported():
    m = _mod()
    for s in ("fasim_score_mutagenesis", "fasim_mutagenesis_tsv"):
        assert s in m.EXPORTS and hasattr(m.lib(), s)
    for name in ("mutagenesis_tsv", "mutagenesis_variants"):
        assert callable(getattr(m, name))
    assert callable(m.Engine.score_mutagenesis)
    hdr = open(os.path.join(entry.ROOT, "include", "fasim_hip.h")).read()
    for word in ("fasim_interval", "fasim_mut_score", "fasim_mutagenesis_stats", "fasim_score_mutagenesis", "fasim_mutagenesis_tsv"):
        assert word in hdr


HEAD = "line\tchrom\tpos\tid\tref\talt" + "".join(f"\t{c}_ref\t{c}_alt" for c in CLASS_NAMES) + "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n"


def test_mutagenesis_tsv_bytes():
    """Three positions of one interval and an interval that was not scored: a position whose byte is none of ACGT (no lines), one
    whose reference letter has value 0 (NA rule) and a clipped line; the clip flag is the bit of the larger of the two letters'
    words, and a tie goes to the bit."""
    m = _mod()
    regions = [m.Region(4, "chr1", 99, 102, "site"), m.Region(6, "chr2", 5, 9, "lost")]
    values = np.zeros((3, 4, 4), dtype=np.int32)
    encs = np.full((3, 4, 4), -1, dtype=np.int8)
    ref = np.array([2, -1, 0], dtype=np.int8)
    clipped = np.zeros((3, 4), dtype=np.uint8)
    values[0, 2] = [50, 0, 75, 60]; encs[0, 2] = [2, -1, 16, 13]          # ref G: max 75, enc 16 -> rule 3
    values[0, 0] = [41, 0, 84, 60]; encs[0, 0] = [2, -1, 18, 47]          # A: max 84, enc 18 -> rule 4
    values[0, 1] = [0, 20, 75, 0]; encs[0, 1] = [-1, 11, 14, -1]          # C: max 75 (enc 14 -> rule 2), clipped: a tie with the unclipped ref
    clipped[0, 1] = 1
    values[0, 3] = [10, 0, 0, 0]; encs[0, 3] = [0, -1, -1, -1]            # T: below the ref, clipped, which does not count
    clipped[0, 3] = 1
    values[1] = 999                                                       # ref -1: never printed
    values[2, 1] = [0, 20, 0, 0]; encs[2, 1] = [-1, 11, -1, -1]           # ref A has value 0; C: enc 11 -> rule 6
    got = m.mutagenesis_tsv(regions, values, encs, ref, clipped, [0, 3, 3], 300, "MEG3")
    want = ("# fasim mutagenesis lncRNA=MEG3 flank=300\n" + HEAD +
            "4\tchr1\t100\tsite\tG\tA\t50\t41\t0\t0\t75\t84\t60\t60\t75\t84\t9\t3\t4\t0\n"
            "4\tchr1\t100\tsite\tG\tC\t50\t0\t0\t20\t75\t75\t60\t0\t75\t75\t0\t3\t2\t1\n"
            "4\tchr1\t100\tsite\tG\tT\t50\t10\t0\t0\t75\t0\t60\t0\t75\t10\t-65\t3\t1\t0\n"
            "4\tchr1\t102\tsite\tA\tC\t0\t0\t0\t20\t0\t0\t0\t0\t0\t20\t20\tNA\t6\t0\n"
            "4\tchr1\t102\tsite\tA\tG" + "\t0" * 11 + "\tNA\tNA\t0\n"
            "4\tchr1\t102\tsite\tA\tT" + "\t0" * 11 + "\tNA\tNA\t0\n")
    assert got == want.encode()
    assert m.mutagenesis_tsv([], np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), np.zeros(0), np.zeros((0, 4)), [0], 0, "q") == \
        ("# fasim mutagenesis lncRNA=q flank=0\n" + HEAD).encode()


def test_mutagenesis_variants_names_the_same_snvs():
    m = _mod()
    dnas = [b"ACNgT", b"GG"]
    got = m.mutagenesis_variants([(0, 1, 5), (1, 0, 1)], dnas)
    assert [tuple(v) for v in got] == [
        (1, "rec0", 1, ".", "C", "A", 0, True), (1, "rec0", 1, ".", "C", "G", 0, True), (1, "rec0", 1, ".", "C", "T", 0, True),
        (1, "rec0", 4, ".", "T", "A", 0, True), (1, "rec0", 4, ".", "T", "C", 0, True), (1, "rec0", 4, ".", "T", "G", 0, True),
        (2, "rec1", 0, ".", "G", "A", 1, True), (2, "rec1", 0, ".", "G", "C", 1, True), (2, "rec1", 0, ".", "G", "T", 1, True)]
    assert m.mutagenesis_variants([], dnas) == []


# ---- the CLI: usage errors and bad files exit 2 before any engine exists and write nothing --------------------------------------
def _cli(tmp_path, *args, bed="chr1\t10\t40\tsite\n"):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    (tmp_path / "r.bed").write_text("chr1\t0\t50\n")
    (tmp_path / "v.vcf").write_text("chr1\t10\trs1\tC\tG\n")
    if bed is not None:
        (tmp_path / "m.bed").write_text(bed)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    return r, sorted(os.listdir(out))


@pytest.mark.parametrize("other", [("--variants", "v.vcf"), ("--regions", "r.bed"), ("--all-records",), ("--accumulate-records",), ("-F",),
                                   ("--track", "25"), ("--all-records", "--screen"), ("--tfo-profile",), ("--sites", "40"),
                                   ("--sites", "40", "--oligos"), ("--potential-hist",), ("--devices", "0")],
                         ids=lambda o: o[-1] if o[-1].startswith("-") else o[0])
def test_cli_mutagenesis_excludes_the_other_products(tmp_path, other):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", *other)
    assert r.returncode == 2, r.stderr
    assert written == []


@pytest.mark.parametrize("flank", ["-1", "2049", "12x", ""])
def test_cli_mutagenesis_flank_out_of_range_exits_2(tmp_path, flank):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", "--mutagenesis-flank", flank)
    assert r.returncode == 2 and "--mutagenesis-flank" in r.stderr, r.stderr
    assert written == []


def test_cli_mutagenesis_flank_needs_mutagenesis(tmp_path):
    r, written = _cli(tmp_path, "--mutagenesis-flank", "100")
    assert r.returncode == 2 and "--mutagenesis-flank needs --mutagenesis" in r.stderr, r.stderr
    assert written == []


@pytest.mark.parametrize("length,flank", [(4521, 300), (5121, 0), (1025, 2048)])
def test_cli_interval_too_long_for_the_flank_names_its_line(tmp_path, length, flank):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", "--mutagenesis-flank", str(flank), bed=f"# c\nchr1\t0\t20\nchr1\t5\t{5 + length}\tbig\n")
    assert r.returncode == 2 and "BED line 3" in r.stderr and "5120" in r.stderr, r.stderr
    assert written == []


BAD_BED = [("chr1\t10\n", 1), ("chr1\t0\t5\nchr1\tx\t9\n", 2), ("chr1\t-1\t9\n", 1), ("chr1\t9\t9\n", 1)]


@pytest.mark.parametrize("text,line", BAD_BED, ids=[str(i) for i in range(len(BAD_BED))])
def test_cli_exits_2_on_a_bad_bed_file(tmp_path, text, line):
    r, written = _cli(tmp_path, "--mutagenesis", "m.bed", bed=text)
    assert r.returncode == 2 and f"line {line}" in r.stderr, r.stderr
    assert written == []


def test_cli_missing_bed_file_exits_2(tmp_path):
    r, written = _cli(tmp_path, "--mutagenesis", "missing.bed", bed=None)
    assert r.returncode == 2 and "missing.bed" in r.stderr, r.stderr
    assert written == []
