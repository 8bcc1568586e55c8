"""Variants scored by the triplex potential through them (fasim_score_variants), the part that needs no GPU: the
yardstick of the GPU tests -- an independent numpy restatement of the touching matrix, tied here to the restatement of section 11
(test_track_cpu.colmax_units) -- and the pure host functions fasim_read_vcf and fasim_variants_tsv, and the CLI's usage errors.

The restatement never calls the code under test.  Per unit (allele window x encoding) it is the Gotoh local alignment of section 11
over the m real rows (no pad rows), column by column over all rows at once, every value carried as 2 * value + b:
    dg = Hdiag + 2 s                       in the columns before v1
    dg = Hdiag + 2 s if Hdiag > 0 else 0   from v1 on (nothing starts afresh behind the allele)
    H' = floor(max(dg, E))                 floor(x) = x if x >= 2 else 0: 0 is "no alignment" and carries no bit
    F[i] = floor(max over k < i of (H'[k] + 8 k) - 8 i - 24)
    H = max(H', F)
    E = floor(max(E - 8, H - 32))
with b OR-ed into the positive cells of a first / last column that the flank cut.  The unit's value is the maximum of H over the
columns from v0 on."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, colmax_units, enabled_encodings, enc_class, encode_unit

CLASS_NAMES = ("ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus")


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(autouse=True)
def _feature():
    """The restatement is the yardstick of a product: without the product's symbols none of these tests has anything to measure."""
    m = _mod()
    assert "fasim_score_variants" in m.EXPORTS and hasattr(m.lib(), "fasim_score_variants")


def _floor(x):
    return np.where(x < 2, 0, x)


def _touch(rna: bytes, targets, v0, v1, edge_lo, edge_hi):
    """(2 * value + b per unit, (units, n) column maxima of H as plain values).  v0, v1, edge_lo, edge_hi: scalars or one per unit;
    edge_lo / edge_hi belong to the unit's first / last column."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    m = len(q)
    t = np.stack([_CODE[np.frombuffer(x, dtype=np.uint8)] for x in targets])
    nu, n = t.shape
    v0 = np.broadcast_to(np.asarray(v0, dtype=np.int64), (nu,))
    v1 = np.broadcast_to(np.asarray(v1, dtype=np.int64), (nu,))
    edge_lo = np.broadcast_to(np.asarray(edge_lo, dtype=bool), (nu,))
    edge_hi = np.broadcast_to(np.asarray(edge_hi, dtype=bool), (nu,))
    prof = np.zeros((5, m), dtype=np.int64)
    for c in range(5):
        prof[c] = np.where((q == c) & (q < 4), 10, -8)
    ramp = 8 * np.arange(m, dtype=np.int64)
    h = np.zeros((nu, m), dtype=np.int64)
    e = np.zeros((nu, m), dtype=np.int64)
    diag = np.zeros((nu, m), dtype=np.int64)
    best = np.zeros(nu, dtype=np.int64)
    cols = np.zeros((nu, n), dtype=np.int64)
    for j in range(n):
        diag[:, 1:] = h[:, :-1]
        dg = diag + prof[t[:, j]]
        cont = (j >= v1)[:, None]
        dg = np.where(cont & (diag == 0), 0, dg)
        mark = (((j == 0) & edge_lo) | ((j == n - 1) & edge_hi))[:, None]
        hp = _floor(np.maximum(dg, e))
        hp = np.where(mark & (hp > 0), hp | 1, hp)
        run = np.maximum.accumulate(hp + ramp, axis=1)
        f = np.zeros_like(hp)
        f[:, 1:] = _floor(run[:, :-1] - ramp[1:] - 24)
        h = np.maximum(hp, f)
        h = np.where(mark & (h > 0), h | 1, h)
        e = _floor(np.maximum(e - 8, h - 32))
        top = h.max(axis=1)
        cols[:, j] = top >> 1
        best = np.where(j >= v0, np.maximum(best, top), best)
    return best, cols


def touch_units(rna: bytes, targets, v0, v1, edge_lo, edge_hi):
    """2 * value + b of the definition for several targets of one length: (len(targets),) int64."""
    return _touch(rna, targets, v0, v1, edge_lo, edge_hi)[0]


def colmax_free(rna: bytes, target: bytes):
    """Column maxima of the plain local matrix over the real rows only (the whole window marked: every column is plain)."""
    if len(target) == 0:
        return np.zeros(0, dtype=np.int64)
    return _touch(rna, [target], 0, len(target), False, False)[1][0]


def touch_scalar(rna: bytes, target: bytes, v0: int, v1: int, edge_lo: bool, edge_hi: bool) -> int:
    """The same as a plain double loop with explicit E and F."""
    q = [int(_CODE[c]) for c in rna]
    m, n = len(q), len(target)

    def fl(x):
        return x if x >= 2 else 0
    h_prev, e_prev = [0] * (m + 1), [0] * (m + 1)
    best = 0
    for j, ch in enumerate(target):
        tc = int(_CODE[ch])
        mark = (j == 0 and edge_lo) or (j == n - 1 and edge_hi)
        h, e = [0] * (m + 1), [0] * (m + 1)
        f = 0
        for i in range(1, m + 1):
            s = 10 if (q[i - 1] == tc and tc < 4) else -8
            e[i] = fl(max(e_prev[i] - 8, h_prev[i] - 32))
            f = fl(max(f - 8, h[i - 1] - 32)) if i > 1 else 0
            d = h_prev[i - 1]
            dg = 0 if (j >= v1 and d == 0) else d + s
            x = fl(max(dg, e[i], f))
            if mark and x > 0:
                x |= 1
            h[i] = x
            if j >= v0:
                best = max(best, x)
        h_prev, e_prev = h, e
    return best


# ---- the whole definition: what Engine.score_variants must return ---------------------------------------------------------------
def windows(dna: bytes, pos: int, ref_len: int, alt: bytes, flank: int):
    """(ref window, alt window, v0, edge_lo, edge_hi) of a variant at 0-based `pos` of record `dna`."""
    lo, hi = max(0, pos - flank), min(len(dna), pos + ref_len + flank)
    ref = dna[lo:hi]
    return ref, dna[lo:pos] + alt + dna[pos + ref_len:hi], pos - lo, lo > 0, hi < len(dna)


def expected_scores(rna: bytes, dnas, variants, flank: int, p):
    """values (nvar, 2, 4), encs (nvar, 2, 4), flags (nvar) of the definition for one query."""
    encs = enabled_encodings(p)
    nvar = len(variants)
    values = np.zeros((nvar, 2, 4), dtype=np.int64)
    which = np.full((nvar, 2, 4), -1, dtype=np.int64)
    flags = np.zeros(nvar, dtype=np.int64)
    # units of one length go through the restatement together
    groups = {}
    for k, v in enumerate(variants):
        if not v.usable:
            continue
        alt = v.alt.encode()
        ref_w, alt_w, v0, e_lo, e_hi = windows(dnas[v.rec], v.pos, len(v.ref), alt, flank)
        for al, (w, alen) in enumerate(((ref_w, len(v.ref)), (alt_w, len(alt)))):
            n, v1 = len(w), v0 + alen
            for e in encs:
                u = (encode_unit(w, e), n - v1, n - v0, e_hi, e_lo) if e & 1 else (encode_unit(w, e), v0, v1, e_lo, e_hi)
                groups.setdefault(n, []).append((k, al, e, u))
    x = {}
    for n, items in groups.items():
        got = touch_units(rna, [u[0] for _, _, _, u in items], [u[1] for _, _, _, u in items], [u[2] for _, _, _, u in items],
                          [u[3] for _, _, _, u in items], [u[4] for _, _, _, u in items])
        for (k, al, e, _), g in zip(items, got):
            x[(k, al, e)] = int(g)
    for k, v in enumerate(variants):
        if not v.usable:
            continue
        top = 0
        for al in range(2):
            for c in range(4):
                mine = [(x[(k, al, e)], e) for e in encs if enc_class(e) == c]
                if not mine:
                    continue
                big = max(w for w, _ in mine)
                top = max(top, big)
                values[k, al, c] = big >> 1
                if big >> 1:
                    which[k, al, c] = min(e for w, e in mine if w >> 1 == big >> 1)
        flags[k] = top & 1
    return values, which, flags


# ---- ties to the existing restatement ---------------------------------------------------------------------------------------------
def _cases():
    """(rna, target, v0, v1): random targets and targets with a planted, gapped copy of a stretch of the query; marks at column 0,
    at the last column, of full width and in between."""
    out = []
    k = 0
    for m in (1, 16, 17, 40, 113):
        for rep in range(60):
            k += 1
            rna = synth.random_rna(m, 1000 + k)
            n = 20 + (k * 7) % 90
            tgt = bytearray(synth.random_dna(n, 2000 + k))
            if rep % 2 and m >= 16:
                a = (k * 5) % max(1, m - 12)
                piece = bytearray(rna[a:a + min(m - a, 12 + k % 30)].replace(b"U", b"A"))
                if rep % 4 == 1 and len(piece) > 8:
                    del piece[len(piece) // 2]                  # a gap in the target
                elif rep % 4 == 3 and len(piece) > 8:
                    piece[len(piece) // 2:len(piece) // 2] = b"CC"      # a gap in the query
                at = (k * 3) % max(1, n - len(piece))
                tgt[at:at + len(piece)] = piece[:n - at]
            tgt = bytes(tgt[:n])
            kind = rep % 6
            if kind == 0:
                v0, v1 = 0, 1
            elif kind == 1:
                v0, v1 = n - 1, n
            elif kind == 2:
                v0, v1 = 0, n
            else:
                v0 = (k * 11) % n
                v1 = min(n, v0 + 1 + (k % 7))
            out.append((rna, tgt, v0, v1))
    return out


def test_restatement_ties_to_the_column_maxima_of_section_11():
    """(a) the whole window marked: the value is the maximum of the (pad-free) column maxima, which is the maximum of
    colmax_units; for 16 rows (no pad rows) the pad-free column maxima are colmax_units' column by column.
    (b) max(colmax[v0:]) == max(T, max(colmax of target[v1:])), and T is strictly smaller in at least 5 % of the cases."""
    cases = _cases()
    smaller = 0
    for rna, tgt, v0, v1 in cases:
        n = len(tgt)
        free = colmax_free(rna, tgt)
        padded = colmax_units(rna, [tgt])[0]
        assert int(free.max()) == int(padded.max())
        if len(rna) % 16 == 0:
            assert free.tolist() == padded.tolist()
        assert int(touch_units(rna, [tgt], 0, n, False, False)[0]) == 2 * int(free.max())
        T = int(touch_units(rna, [tgt], v0, v1, False, False)[0])
        assert T & 1 == 0
        T >>= 1
        suffix = colmax_free(rna, tgt[v1:])
        rest = int(suffix.max()) if len(suffix) else 0
        assert int(free[v0:].max()) == max(T, rest), (rna, tgt, v0, v1)
        smaller += T < int(free[v0:].max())
    print(f"{smaller} of {len(cases)} cases have a touching value below the maximum from the variant on")
    assert smaller * 20 >= len(cases)


def test_vectorised_form_equals_the_double_loop():
    """(c) bit included, with every combination of cut ends."""
    for i, (rna, tgt, v0, v1) in enumerate(_cases()[::3]):
        e_lo, e_hi = bool(i & 1), bool(i & 2)
        got = int(touch_units(rna, [tgt], v0, v1, e_lo, e_hi)[0])
        assert got == touch_scalar(rna, tgt, v0, v1, e_lo, e_hi), (rna, tgt, v0, v1, e_lo, e_hi)
    # several units of one length at once, each with its own mark and ends
    rna = synth.random_rna(40, 77)
    tg = [synth.random_dna(64, 300 + k) for k in range(6)]
    v0 = [0, 5, 63, 10, 30, 0]
    v1 = [1, 9, 64, 64, 31, 64]
    lo = [True, False, True, False, True, True]
    hi = [False, True, True, False, True, False]
    assert touch_units(rna, tg, v0, v1, lo, hi).tolist() == [touch_scalar(rna, tg[k], v0[k], v1[k], lo[k], hi[k]) for k in range(6)]


def test_clip_bit_marks_alignments_that_reach_a_cut_end():
    rna = b"AGGAGAAGGAGAGGAAGAGA"
    tgt = b"CCCCCCCCCC" + rna + b"TTTTTTTTTT"
    n = len(tgt)
    # the copy ends well inside the window: no bit, whatever the ends
    assert int(touch_units(rna, [tgt], 15, 16, True, True)[0]) == 2 * 100
    # the window is cut in the middle of the copy: its best alignment starts in the first / ends in the last column
    assert int(touch_units(rna, [tgt[15:]], 3, 4, True, False)[0]) == 2 * 75 + 1
    assert int(touch_units(rna, [tgt[15:]], 3, 4, False, False)[0]) == 2 * 75
    assert int(touch_units(rna, [tgt[:n - 15]], 12, 13, False, True)[0]) == 2 * 75 + 1
    assert int(touch_units(rna, [tgt[:n - 15]], 12, 13, True, False)[0]) == 2 * 75


def test_a_repaired_mismatch_is_worth_nine():
    """(d) a planted 30-mer with one mismatch in the variant column: +9 for the allele that repairs it, -9 for the reverse."""
    rna = synth.random_rna(40, 4242).replace(b"U", b"A")
    good = rna[5:35]
    col = 14
    bad = bytearray(good)
    bad[col] = {65: 67, 67: 71, 71: 84, 84: 65}[bad[col]]
    left, right = b"N" * 24, b"N" * 24      # (N never matches: the copy cannot be extended)
    ref_t, alt_t = left + bytes(bad) + right, left + good + right
    v0 = len(left) + col
    ref_v, alt_v = (int(touch_units(rna, [t], v0, v0 + 1, True, True)[0]) >> 1 for t in (ref_t, alt_t))
    assert (ref_v, alt_v) == (141, 150)
    assert alt_v - ref_v == 9 and ref_v - alt_v == -9
    # and through the whole definition: encoding 0 maps A, T, G, C to T, G, G, T, so the pre-image of the query is planted on the DNA side
    m = _mod()
    q = b"TGGTTGTGGTGTTGGTGGTTGTGTGGTTGT"
    pre = q.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A")
    assert encode_unit(pre, 0) == q
    dna = b"N" * 50 + pre + b"N" * 50
    at = 50 + 11
    ref = dna[at:at + 1]
    alt = b"T" if ref == b"A" else b"A"
    p = m.default_params(rule=1, strand=1)
    vals, which, flags = expected_scores(q, [dna], [m.Variant(1, "c", at, ".", ref.decode(), alt.decode())], 40, p)
    assert vals[0, 0, 0] == 150 and vals[0, 1, 0] == 141 and which[0, 0, 0] == 0 and flags[0] == 0


# ---- fasim_read_vcf -----------------------------------------------------------------------------------------------------------------
def _vcf(tmp_path, text, name="v.vcf"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_read_vcf_lines_alleles_and_skipped_kinds(tmp_path):
    m = _mod()
    text = ("##fileformat=VCFv4.2\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "\n"
            "chr1\t10\trs1\ta\tg\t50\tPASS\tDP=3\n"                      # upper-cased, further columns ignored
            "chr1\t20\t.\tAC\tA,ACGT,<DEL>\n"                            # one entry per ALT allele, same line
            "chr2\t5\trs3\tG\t*\r\n"                                     # CRLF; a `*` allele
            "chr2\t6\trs4\tG\t.\n"
            "chr2\t7\tbnd\tG\tG]17:198982]\n"                            # a breakend
            "chr2\t8\tiupac\tG\tR\n"                                     # letters outside ACGTN
            "chr2\t9\tn\tN\tT\n"
            "chr2\t11\tlong\tG\t" + "A" * (m.MAX_ALLELE + 1) + "\n"
            "chr2\t12\tmax\tG\t" + "A" * m.MAX_ALLELE + "\n")
    got = m.read_vcf(_vcf(tmp_path, text))
    assert [tuple(v) for v in got[:9]] == [
        (4, "chr1", 9, "rs1", "A", "G", 0, True),
        (5, "chr1", 19, ".", "AC", "A", 0, True),
        (5, "chr1", 19, ".", "AC", "ACGT", 0, True),
        (5, "chr1", 19, ".", "AC", "<DEL>", 0, False),
        (6, "chr2", 4, "rs3", "G", "*", 0, False),
        (7, "chr2", 5, "rs4", "G", ".", 0, False),
        (8, "chr2", 6, "bnd", "G", "G]17:198982]", 0, False),
        (9, "chr2", 7, "iupac", "G", "R", 0, False),
        (10, "chr2", 8, "n", "N", "T", 0, True),
    ]
    assert (got[9].line, got[9].usable, len(got[9].alt)) == (11, False, m.MAX_ALLELE + 1)
    assert (got[10].line, got[10].usable, len(got[10].alt)) == (12, True, m.MAX_ALLELE)
    assert len(got) == 11
    assert m.read_vcf(_vcf(tmp_path, "# nothing\n\n")) == []
    assert m.MAX_ALLELE == 1024 and m.MAX_FLANK == 2048


BAD_VCF = [
    ("chr1\t10\trs1\tA\n", 1, "fewer than 5 columns"),
    ("#h\nchr1\t10\trs1\tA\tG\nchr1 11 rs2 A G\n", 3, "fewer than 5 columns"),
    ("chr1\tten\trs1\tA\tG\n", 1, "not an integer"),
    ("chr1\t1.5\trs1\tA\tG\n", 1, "not an integer"),
    ("chr1\t5\trs1\tA\tG\nchr1\t0\trs1\tA\tG\n", 2, "POS 0 < 1"),
    ("chr1\t-3\trs1\tA\tG\n", 1, "POS -3 < 1"),
    ("chr1\t5\trs1\t\tG\n", 1, "empty REF"),
    ("chr1\t5\trs1\tA\t\n", 1, "empty ALT"),
    ("##x\nchr1\t5\trs1\tA\tG,,T\n", 2, "empty ALT"),
]


@pytest.mark.parametrize("text,line,reason", BAD_VCF, ids=[b[2].split()[0] + str(i) for i, b in enumerate(BAD_VCF)])
def test_read_vcf_refusals_name_the_line_and_the_reason(tmp_path, text, line, reason):
    m = _mod()
    with pytest.raises(m.FasimError) as ei:
        m.read_vcf(_vcf(tmp_path, text))
    assert ei.value.code == m.E_ARG
    assert f"line {line}:" in str(ei.value) and reason in str(ei.value), str(ei.value)


def test_read_vcf_missing_file_is_refused(tmp_path):
    m = _mod()
    with pytest.raises(m.FasimError) as ei:
        m.read_vcf(str(tmp_path / "missing.vcf"))
    assert ei.value.code == m.E_ARG and "cannot read" in str(ei.value)


# ---- fasim_variants_tsv ------------------------------------------------------------------------------------------------------------
def test_variants_tsv_bytes():
    m = _mod()
    V = m.Variant
    variants = [V(3, "chr1", 99, "rs1", "A", "G"), V(4, "chr1", 199, ".", "AC", "A"), V(4, "chr1", 199, ".", "AC", "<DEL>", 0, False),
                V(7, "chr9", 0, "lost", "T", "C"), V(8, "chr1", 299, "flat", "T", "C")]
    values = np.zeros((5, 2, 4), dtype=np.int32)
    encs = np.full((5, 2, 4), -1, dtype=np.int32)
    flags = np.zeros(5, dtype=np.int32)
    values[0] = [[50, 0, 75, 75], [41, 0, 84, 60]]
    encs[0] = [[2, -1, 16, 13], [2, -1, 18, 47]]          # rules: enc 16 -> 3, enc 18 -> 4
    values[1] = [[0, 20, 0, 0], [0, 0, 0, 0]]
    encs[1] = [[-1, 11, -1, -1], [-1, -1, -1, -1]]        # enc 11 -> rule 6
    flags[1] = 1
    values[3] = 999                                        # not matched: never printed
    got = m.variants_tsv(variants, values, encs, flags, 300, "MEG3", matched=[1, 1, 1, 0, 1])
    head = "line\tchrom\tpos\tid\tref\talt" + "".join(f"\t{c}_ref\t{c}_alt" for c in CLASS_NAMES) + \
           "\tmax_ref\tmax_alt\tdelta\trule_ref\trule_alt\tclipped\n"
    na = "\tNA" * 14 + "\n"
    want = ("# fasim variants lncRNA=MEG3 flank=300\n" + head +
            "3\tchr1\t100\trs1\tA\tG\t50\t41\t0\t0\t75\t84\t75\t60\t75\t84\t9\t3\t4\t0\n"
            "4\tchr1\t200\t.\tAC\tA\t0\t0\t20\t0\t0\t0\t0\t0\t20\t0\t-20\t6\tNA\t1\n"
            "4\tchr1\t200\t.\tAC\t<DEL>" + na +
            "7\tchr9\t1\tlost\tT\tC" + na +
            "8\tchr1\t300\tflat\tT\tC" + "\t0" * 11 + "\tNA\tNA\t0\n")
    assert got == want.encode()
    assert m.variants_tsv([], np.zeros((0, 2, 4)), np.zeros((0, 2, 4)), np.zeros(0), 0, "q") == ("# fasim variants lncRNA=q flank=0\n" + head).encode()


def test_variant_symbols_are_exported():
    m = _mod()
    for s in ("fasim_read_vcf", "fasim_score_variants", "fasim_variants_tsv"):
        assert s in m.EXPORTS and hasattr(m.lib(), s)
    for name in ("MAX_ALLELE", "MAX_FLANK", "read_vcf", "variants_tsv", "Variant"):
        assert hasattr(m, name)
    assert callable(m.Engine.score_variants)
    hdr = open(os.path.join(entry.ROOT, "include", "fasim_hip.h")).read()
    assert "#define FASIM_MAX_ALLELE 1024" in hdr and "#define FASIM_MAX_FLANK  2048" in hdr


# ---- the CLI: usage errors and bad files exit 2 before any engine exists and write nothing --------------------------------------
def _cli(tmp_path, *args):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    (tmp_path / "r.bed").write_text("chr1\t0\t50\n")
    if not (tmp_path / "v.vcf").exists():
        (tmp_path / "v.vcf").write_text("chr1\t10\trs1\tC\tG\n")
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    return r, sorted(os.listdir(out))


@pytest.mark.parametrize("other", [("--regions", "r.bed"), ("--all-records",), ("--accumulate-records",), ("-F",), ("--track", "25"),
                                   ("--all-records", "--screen"), ("--tfo-profile",), ("--sites", "40"),
                                   ("--sites", "40", "--oligos"), ("--potential-hist",), ("--devices", "0")],
                         ids=lambda o: o[-1] if o[-1].startswith("-") else o[0])
def test_cli_variants_excludes_the_other_products(tmp_path, other):
    r, written = _cli(tmp_path, "--variants", "v.vcf", *other)
    assert r.returncode == 2, r.stderr
    assert written == []


@pytest.mark.parametrize("flank", ["-1", "2049", "12x", ""])
def test_cli_variant_flank_out_of_range_exits_2(tmp_path, flank):
    r, written = _cli(tmp_path, "--variants", "v.vcf", "--variant-flank", flank)
    assert r.returncode == 2 and "--variant-flank" in r.stderr, r.stderr
    assert written == []


def test_cli_variant_flank_needs_variants(tmp_path):
    r, written = _cli(tmp_path, "--variant-flank", "100")
    assert r.returncode == 2 and "--variant-flank needs --variants" in r.stderr, r.stderr
    assert written == []


@pytest.mark.parametrize("text,line,reason", BAD_VCF, ids=[b[2].split()[0] + str(i) for i, b in enumerate(BAD_VCF)])
def test_cli_exits_2_on_a_bad_vcf_file(tmp_path, text, line, reason):
    _vcf(tmp_path, text)
    r, written = _cli(tmp_path, "--variants", "v.vcf")
    assert r.returncode == 2, r.stderr
    assert f"line {line}:" in r.stderr and reason in r.stderr, r.stderr
    assert written == []


def test_cli_missing_vcf_file_exits_2(tmp_path):
    r, written = _cli(tmp_path, "--variants", "missing.vcf")
    assert r.returncode == 2 and "cannot read VCF file" in r.stderr, r.stderr
    assert written == []
