"""The alignment behind every variant score (fasim_score_variants_aligned), the part that needs no GPU: the
yardstick of the GPU tests -- an independent restatement of the hit's definition, which never calls the code under test --, the pure
host functions fasim_variant_hit_span and fasim_variant_hits_tsv, and the CLI's usage errors.

The restatement keeps the whole matrices T, E and F of a unit in plain values (+5 / -4, first gap residue 16, each further one 4),
columns vectorised over the rows as test_variants_cpu._touch does:
    E[i][j] = max(E[i][j-1] - 4, T[i][j-1] - 16, 0)
    dg      = d + s, with d = T[i-1][j-1]; from v1 on 0 where d == 0
    T'      = max(dg, E, 0)
    F[i][j] = max over k < i of T'[k][j] - 16 - 4 (i - 1 - k), floored at 0
    T       = max(T', F)
and walks the path back with a scalar loop: end cell = smallest column >= v0, then smallest row, that holds the value; in H: the
diagonal where d > 0 and T == d + s, else the first pair where d == 0, j < v1 and T == s, else E where T == E, else F; in a gap state
extend before open."""
import os
import re
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, enabled_encodings, encode_unit
from test_site_align_cpu import rescore, triplex_record
from test_variants_cpu import _cases, expected_scores, touch_scalar, touch_units, windows


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(autouse=True)
def _feature():
    """Without the product's symbols none of these tests has anything to measure."""
    m = _mod()
    assert "fasim_score_variants_aligned" in m.EXPORTS and hasattr(m.lib(), "fasim_score_variants_aligned")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def touch_matrices(rna: bytes, target: bytes, v0: int, v1: int):
    """T, E, F of one unit: (m, n) int32 arrays of plain values."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = _CODE[np.frombuffer(target, dtype=np.uint8)]
    m, n = len(q), len(t)
    prof = np.zeros((5, m), dtype=np.int32)
    for c in range(5):
        prof[c] = np.where((q == c) & (q < 4), 5, -4)
    ramp = 4 * np.arange(m, dtype=np.int32)
    T = np.zeros((m, n), dtype=np.int32)
    E = np.zeros((m, n), dtype=np.int32)
    F = np.zeros((m, n), dtype=np.int32)
    h = np.zeros(m, dtype=np.int32)
    e = np.zeros(m, dtype=np.int32)
    diag = np.zeros(m, dtype=np.int32)
    for j in range(n):
        diag[1:] = h[:-1]
        dg = diag + prof[t[j]]
        if j >= v1:
            dg = np.where(diag == 0, 0, dg)
        e = np.maximum(np.maximum(e - 4, h - 16), 0)
        hp = np.maximum(np.maximum(dg, e), 0)
        f = np.zeros(m, dtype=np.int32)
        f[1:] = np.maximum(np.maximum.accumulate(hp + ramp)[:-1] - ramp[1:] - 12, 0)
        h = np.maximum(hp, f)
        T[:, j], E[:, j], F[:, j] = h, e, f
    return T, E, F


def trace(rna: bytes, target: bytes, T, E, F, v0: int, v1: int, value: int):
    """(i0, i1, j0, j1, cigar string) of the definition; every step asserts that the matrices explain the cell."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = _CODE[np.frombuffer(target, dtype=np.uint8)]
    cols = np.flatnonzero((T[:, v0:] == value).any(axis=0))
    assert len(cols), "the value is not in the matrix"
    j1 = v0 + int(cols[0])
    i1 = int(np.flatnonzero(T[:, j1] == value)[0])
    i, j, state, ops = i1, j1, "H", []
    while True:
        assert i >= 0 and j >= 0
        if state == "H":
            d = int(T[i - 1, j - 1]) if i > 0 and j > 0 else 0
            s = 5 if (q[i] == t[j] and t[j] < 4) else -4
            x = int(T[i, j])
            assert x > 0
            if d > 0 and x == d + s:
                ops.append("M"); i -= 1; j -= 1
            elif d == 0 and j < v1 and x == s:
                ops.append("M")
                break
            elif x == int(E[i, j]):
                state = "E"
            else:
                assert x == int(F[i, j])
                state = "F"
        elif state == "E":
            ops.append("D")
            assert j > 0
            if int(E[i, j]) != int(E[i, j - 1]) - 4:
                assert int(E[i, j]) == int(T[i, j - 1]) - 16
                state = "H"
            j -= 1
        else:
            ops.append("I")
            assert i > 0
            if int(F[i, j]) != int(F[i - 1, j]) - 4:
                assert int(F[i, j]) == int(T[i - 1, j]) - 16
                state = "H"
            i -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    return i, i1, j, j1, "".join(f"{n}{o}" for n, o in runs)


def unit_hit(rna: bytes, target: bytes, v0: int, v1: int, value: int):
    T, E, F = touch_matrices(rna, target, v0, v1)
    assert int(T[:, v0:].max()) == value
    return trace(rna, target, T, E, F, v0, v1, value)


def span_ref(pos: int, ref_len: int, alen: int, pre: int, post: int, enc: int, j0: int, j1: int):
    """Step 6 of the definition, written out."""
    n = pre + alen + post
    w0, w1 = (n - 1 - j1, n - 1 - j0) if enc & 1 else (j0, j1)
    if w0 < pre:
        start = pos - pre + w0
    elif w0 < pre + alen:
        start = pos
    else:
        start = pos + ref_len + (w0 - pre - alen)
    if w1 < pre:
        end = pos - pre + w1 + 1
    elif w1 < pre + alen:
        end = pos + ref_len
    else:
        end = pos + ref_len + (w1 - pre - alen) + 1
    return start, end


def expected_hits(rna: bytes, dnas, variants, flank: int, p, scores=None):
    """What Engine.score_variants_aligned must return for one query: (scores, windows (nvar, 3), slots) with slots[(v, allele, cls)] =
    dict(enc, i0, i1, j0, j1, cigar, clipped, n, rec) for every slot with a value.  `scores`: expected_scores of the same call where
    the caller has them already."""
    values, which, flags = scores if scores is not None else expected_scores(rna, dnas, variants, flank, p)
    wins = np.zeros((len(variants), 3), dtype=np.int64)
    slots = {}
    for k, v in enumerate(variants):
        if not v.usable:
            continue
        alt = v.alt.encode()
        d = dnas[v.rec]
        ref_w, alt_w, v0, e_lo, e_hi = windows(d, v.pos, len(v.ref), alt, flank)
        lo = max(0, v.pos - flank)
        wins[k] = (v0, len(ref_w) - v0 - len(v.ref), int(e_lo) | (int(e_hi) << 1))
        for al, (w, alen) in enumerate(((ref_w, len(v.ref)), (alt_w, len(alt)))):
            n, v1 = len(w), v0 + alen
            for c in range(4):
                value, enc = int(values[k, al, c]), int(which[k, al, c])
                if value <= 0:
                    continue
                u0, u1, first, last = (n - v1, n - v0, e_hi, e_lo) if enc & 1 else (v0, v1, e_lo, e_hi)
                i0, i1, j0, j1, cigar = unit_hit(rna, encode_unit(w, enc), u0, u1, value)
                rec = triplex_record(rna, w, enc, lo, value, i0, i1, j0, j1, cigar, p)
                rec["seg"] = k
                slots[(k, al, c)] = dict(enc=enc, i0=i0, i1=i1, j0=j0, j1=j1, cigar=cigar, n=n, rec=rec,
                                         clipped=bool((j0 == 0 and first) or (j1 == n - 1 and last)))
    return (values, which, flags), wins, slots


# ---- the restatement on the cases of section 19 -------------------------------------------------------------------------------------
def test_traced_paths_rescore_to_the_value_and_touch_the_mark():
    ends_d = ends_i = traced = 0
    for rna, tgt, v0, v1 in _cases():
        value2 = int(touch_units(rna, [tgt], v0, v1, False, False)[0])
        assert value2 == touch_scalar(rna, tgt, v0, v1, False, False) and value2 & 1 == 0
        value = value2 >> 1
        if value == 0:
            continue
        T, E, F = touch_matrices(rna, tgt, v0, v1)
        assert 2 * int(T[:, v0:].max()) == value2
        i0, i1, j0, j1, cigar = trace(rna, tgt, T, E, F, v0, v1, value)
        traced += 1
        assert rescore(rna, tgt, i0, j0, cigar) == (value, i1, j1), (rna, tgt, v0, v1, cigar)
        assert j0 < v1 and j1 >= v0
        ops = re.findall(r"[MID]", cigar)
        assert ops[0] == "M"
        ends_d += ops[-1] == "D"
        ends_i += ops[-1] == "I"
    print(f"{traced} paths, {ends_d} end in D, {ends_i} end in I")
    assert traced > 200 and ends_d >= 1 and ends_i == 0


def test_an_allele_reached_only_through_a_gap_ends_in_d():
    rna = b"AGGAGAAGGAGAGGAAGAGA"
    tgt = b"CCCCC" + rna + b"CCCCC"
    assert int(touch_units(rna, [tgt], 25, 26, False, False)[0]) == 2 * 84
    assert unit_hit(rna, tgt, 25, 26, 84) == (0, 19, 5, 25, "20M1D")
    # the mark on the copy's last base: the plain alignment
    assert unit_hit(rna, tgt, 24, 25, 100) == (0, 19, 5, 24, "20M")


# ---- fasim_variant_hit_span ---------------------------------------------------------------------------------------------------------
SPANS = [  # (ref, alt, allele, enc, j0, j1, start, end) at pos 100 with 10 letters on either side
    ("A", "C", 0, 0, 3, 15, 93, 106), ("A", "C", 1, 0, 3, 15, 93, 106), ("A", "C", 1, 0, 10, 10, 100, 101), ("A", "C", 1, 1, 5, 17, 93, 106),
    ("A", "ACGCG", 1, 0, 2, 7, 92, 98),        # before the allele
    ("A", "ACGCG", 1, 0, 3, 12, 93, 101),      # into the allele
    ("A", "ACGCG", 1, 0, 11, 13, 100, 101),    # inside it
    ("A", "ACGCG", 1, 0, 12, 20, 100, 107),    # out of it
    ("A", "ACGCG", 1, 0, 16, 24, 102, 111),    # behind it
    ("A", "ACGCG", 1, 0, 0, 24, 90, 111),      # across it
    ("A", "ACGCG", 1, 1, 4, 21, 93, 107),      # mirrored: w = 24 - j
    ("A", "ACGCG", 1, 13, 0, 8, 102, 111),
    ("A", "ACGCG", 0, 0, 3, 15, 93, 106),      # the REF window: the identity
    ("ACGTAC", "A", 1, 0, 5, 10, 95, 106), ("ACGTAC", "A", 1, 0, 11, 15, 106, 111), ("ACGTAC", "A", 1, 0, 10, 10, 100, 106),
    ("ACGTAC", "A", 1, 0, 2, 8, 92, 99), ("ACGTAC", "A", 1, 1, 5, 9, 106, 111), ("ACGTAC", "A", 1, 1, 10, 20, 90, 106),
    ("ACGTAC", "A", 0, 0, 3, 22, 93, 113), ("ACGTAC", "A", 0, 1, 3, 22, 93, 113),
]


@pytest.mark.parametrize("ref,alt,allele,enc,j0,j1,start,end", SPANS)
def test_variant_hit_span(ref, alt, allele, enc, j0, j1, start, end):
    m = _mod()
    v = m.Variant(1, "c", 100, ".", ref, alt)
    alen = len(alt) if allele else len(ref)
    assert span_ref(100, len(ref), alen, 10, 10, enc, j0, j1) == (start, end)
    assert m.variant_hit_span(v, (10, 10, 0), allele, enc, j0, j1) == (start, end)


def test_variant_hit_span_clipped_and_refusals():
    m = _mod()
    v = m.Variant(1, "c", 100, ".", "A", "ACGCG")
    # edge bit 0: the lower end of the window was cut; an odd encoding has that end in its last column
    assert m.variant_hit_clipped(v, (10, 10, 1), 1, 0, 0, 5) and not m.variant_hit_clipped(v, (10, 10, 1), 1, 0, 1, 24)
    assert m.variant_hit_clipped(v, (10, 10, 1), 1, 1, 3, 24) and not m.variant_hit_clipped(v, (10, 10, 1), 1, 1, 0, 23)
    assert m.variant_hit_clipped(v, (10, 10, 2), 1, 0, 3, 24) and m.variant_hit_clipped(v, (10, 10, 2), 1, 1, 0, 2)
    assert not m.variant_hit_clipped(v, (10, 10, 0), 1, 0, 0, 24)
    for bad in ((1, 0, 5, 25), (1, 0, -1, 3), (1, 0, 6, 5), (2, 0, 1, 2), (1, 48, 1, 2), (0, 0, 0, 21)):
        with pytest.raises(m.FasimError) as ei:
            m.variant_hit_span(v, (10, 10, 0), *bad)
        assert ei.value.code == m.E_ARG


# ---- fasim_variant_hits_tsv ---------------------------------------------------------------------------------------------------------
HEAD = ("line\tchrom\tpos\tid\tref\talt\tallele\tclass\tvalue\trule\tstrand\ttts_start\ttts_end\ttfo_start\ttfo_end\tnt\tidentity\t"
        "stability\tcigar\tclipped\tTFO\tTTS\n")


def test_variant_hits_tsv_of_empty_hits_is_the_two_header_lines():
    m = _mod()
    V = m.Variant
    variants = [V(3, "chr1", 99, "rs1", "A", "G"), V(4, "chr1", 199, ".", "AC", "<DEL>", 0, False)]
    values = np.zeros((2, 2, 4), dtype=np.int32)
    encs = np.full((2, 2, 4), -1, dtype=np.int32)
    wins = np.zeros((2, 3), dtype=np.int32)
    hits = m.empty_variant_hits(2)
    assert hits.n == 16 and hits.unaligned == 0 and hits.cigars() == [""] * 16
    assert hits.array()[:, 2:].tolist() == [[-1, -1, -1, -1, 0, 0]] * 16
    got = m.variant_hits_tsv(variants, values, encs, wins, hits, 300, "MEG3")
    assert got == ("# fasim variant hits lncRNA=MEG3 flank=300\n" + HEAD).encode()
    assert m.variant_hits_tsv([], values[:0], encs[:0], wins[:0], m.empty_variant_hits(0), 0, "q") == \
        ("# fasim variant hits lncRNA=q flank=0\n" + HEAD).encode()
    # a value whose hit is missing keeps its line, NA from tts_start on; an entry that is not matched has no line
    values[0, 1, 2], encs[0, 1, 2] = 84, 18                  # enc 18 -> rule 4, AntiMinus
    want = "3\tchr1\t100\trs1\tA\tG\talt\tAntiMinus\t84\t4\t-" + "\tNA" * 11 + "\n"
    assert m.variant_hits_tsv(variants, values, encs, wins, hits, 300, "MEG3") == ("# fasim variant hits lncRNA=MEG3 flank=300\n" + HEAD + want).encode()
    assert m.variant_hits_tsv(variants, values, encs, wins, hits, 300, "MEG3", matched=[0, 1]) == ("# fasim variant hits lncRNA=MEG3 flank=300\n" + HEAD).encode()
    with pytest.raises(m.FasimError):
        m.variant_hits_tsv(variants, values, encs, wins, m.empty_variant_hits(1), 300, "MEG3")


def test_variant_hit_symbols_are_exported():
    m = _mod()
    for s in ("fasim_score_variants_aligned", "fasim_variant_hit_span", "fasim_variant_hits_tsv"):
        assert s in m.EXPORTS and hasattr(m.lib(), s)
    for name in ("variant_hit_index", "variant_hit_span", "variant_hit_clipped", "variant_hits_tsv", "empty_variant_hits"):
        assert hasattr(m, name)
    assert callable(m.Engine.score_variants_aligned)
    assert [m.variant_hit_index(v, a, c) for v, a, c in ((0, 0, 0), (0, 1, 0), (3, 1, 2))] == [0, 4, 30]
    hdr = open(os.path.join(entry.ROOT, "include", "fasim_hip.h")).read()
    assert "typedef struct fasim_variant_window { int32_t pre, post, edge, reserved; } fasim_variant_window;" in hdr


# ---- the CLI: usage errors exit 2 before any engine exists and write nothing --------------------------------------------------------
def _cli(tmp_path, *args):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    (tmp_path / "v.vcf").write_text("chr1\t10\trs1\tC\tG\n")
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    return r, sorted(os.listdir(out))


def test_cli_variant_hits_needs_variants(tmp_path):
    r, written = _cli(tmp_path, "--variant-hits")
    assert r.returncode == 2 and "--variant-hits needs --variants" in r.stderr, r.stderr
    assert written == []


def test_cli_variant_hits_keeps_the_exclusions_of_variants(tmp_path):
    r, written = _cli(tmp_path, "--variants", "v.vcf", "--variant-hits", "--devices", "0")
    assert r.returncode == 2 and "--variants is not available with" in r.stderr, r.stderr
    assert written == []
