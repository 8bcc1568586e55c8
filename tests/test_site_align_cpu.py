"""Site hits (fasim_scan_records_sites_aligned), the part that needs no GPU: the yardstick of the GPU tests -- a numpy restatement
of the definition in DESIGN.md section 15, site_hit() / site_hits(), which never calls the code under test -- checked here against
a scalar triple-matrix implementation of the same definition, against its own consequence (a) on the demo and against the
reference's ssw_align through the oracle; and the pure host functions of the C-ABI, fasim_site_hits_merge and fasim_site_hits_tsv.

The restatement keeps one unit's whole matrix H (pad rows included) for all the sites of that unit:
    unit    the selected segment of the smallest index that covers pos and whose unit under enc has column maximum value at pos
    end     (i1, j1): the largest column j1 <= jp at which a real row holds H == value, the smallest such row
    start   (i0, j0): G[i][j] = best score of an alignment that begins with the pair (i, j) and ends with the pair (i1, j1), no
            floor; the largest column with some G == value, the largest such row
    path    anchored Gotoh matrices Ha / Ea / Fa of the rectangle, traceback with fixed priorities (H: diagonal, E, F; in a gap
            state: extend, then open)
    record  convertMyTriplex's numbers with ntMin = 1 and no ntMax, float32 left-to-right arithmetic, and the two strings."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, enabled_encodings, enc_class, encode_unit, same_seq
from test_sites_cpu import expected_potential, sites_from

NEG = -(10 ** 6)


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _profile(rna: bytes, rows: int):
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    prof = np.zeros((5, rows), dtype=np.int64)
    for c in range(5):
        prof[c, :len(q)] = np.where((q == c) & (q < 4), 5, -4)
    return prof


def unit_matrix(rna: bytes, target: bytes):
    """H of section 11 for one unit, (16 ceil(m / 16), n) int32: the column loop of colmax_units with every column kept."""
    m = len(rna)
    rows = 16 * ((m + 15) // 16)
    prof = _profile(rna, rows)
    t = _CODE[np.frombuffer(target, dtype=np.uint8)]
    ramp = 4 * np.arange(rows, dtype=np.int64)
    h = np.zeros(rows, dtype=np.int64)
    e = np.zeros(rows, dtype=np.int64)
    diag = np.zeros(rows, dtype=np.int64)
    out = np.zeros((rows, len(t)), dtype=np.int32)
    for j in range(len(t)):
        diag[1:] = h[:-1]
        hp = np.maximum(np.maximum(diag + prof[t[j]], e), 0)
        run = np.maximum.accumulate(hp + ramp)
        f = np.zeros_like(hp)
        f[1:] = run[:-1] - ramp[1:] - 12
        h = np.maximum(hp, f)
        e = np.maximum(np.maximum(e - 4, h - 16), 0)
        out[:, j] = h
    return out


def _anchored(s):
    """Anchored Gotoh matrices of a score rectangle s (rows, cols): Ha[0][0] = s[0][0], nothing else starts, no floor.  Returns
    (Ha, Ea, Fa, D) with D[i][j] = Ha[i-1][j-1] + s[i][j], the score of the best path that ends with the pair (i, j)."""
    rows, cols = s.shape
    ramp = 4 * np.arange(rows, dtype=np.int64)
    ha = np.full((rows, cols), NEG, dtype=np.int64)
    ea = np.full((rows, cols), NEG, dtype=np.int64)
    fa = np.full((rows, cols), NEG, dtype=np.int64)
    dd = np.full((rows, cols), NEG, dtype=np.int64)
    h = np.full(rows, NEG, dtype=np.int64)
    e = np.full(rows, NEG, dtype=np.int64)
    for j in range(cols):
        diag = np.full(rows, NEG, dtype=np.int64)
        diag[1:] = h[:-1]
        if j == 0:
            diag[0] = 0
        e = np.maximum(np.maximum(e - 4, h - 16), NEG)
        d = np.maximum(diag + s[:, j], NEG)
        hp = np.maximum(d, e)
        run = np.maximum.accumulate(hp + ramp)
        f = np.full(rows, NEG, dtype=np.int64)
        f[1:] = np.maximum(run[:-1] - ramp[1:] - 12, NEG)
        h = np.maximum(hp, f)
        ha[:, j], ea[:, j], fa[:, j], dd[:, j] = h, e, f, d
    return ha, ea, fa, dd


def _traceback(ha, ea, fa, dd):
    """The path of the definition from the last cell in state H back to (0, 0), as a list of (length, op) runs, first run first."""
    i, j = ha.shape[0] - 1, ha.shape[1] - 1
    ops, state = [], "H"
    while True:
        if state == "H":
            if ha[i, j] == dd[i, j]:
                ops.append("M")
                if i == 0 and j == 0:
                    break
                i, j = i - 1, j - 1
                assert i >= 0 and j >= 0
            elif ha[i, j] == ea[i, j]:
                state = "E"
            else:
                assert ha[i, j] == fa[i, j]
                state = "F"
        elif state == "E":
            ops.append("D")
            assert j >= 1
            if not ea[i, j] == ea[i, j - 1] - 4:
                assert ea[i, j] == ha[i, j - 1] - 16
                state = "H"
            j -= 1
        else:
            ops.append("I")
            assert i >= 1
            if not fa[i, j] == fa[i - 1, j] - 4:
                assert fa[i, j] == ha[i - 1, j] - 16
                state = "H"
            i -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    return [(n, o) for n, o in runs]


def align_in_unit(rna: bytes, target: bytes, H, jp: int, value: int):
    """Steps 2-4 of the definition in one unit whose column jp has maximum `value`: (i0, i1, j0, j1, cigar string)."""
    m = len(rna)
    rows = H.shape[0]
    prof = _profile(rna, rows)
    t = _CODE[np.frombuffer(target, dtype=np.uint8)]
    assert int(H[:, jp].max()) == value
    hit = np.flatnonzero((H[:m, :jp + 1] == value).any(axis=0))
    j1 = int(hit[-1])
    i1 = int(np.flatnonzero(H[:m, j1] == value)[0])
    # the anchored reverse pass: the rectangle grows towards smaller columns until a column holds a pair that scores `value`
    width = 64
    while True:
        lo = max(0, j1 + 1 - width)
        s = prof[t[lo:j1 + 1]][:, :i1 + 1].T[::-1, ::-1]               # rows i1 .. 0, columns j1 .. lo
        _, _, _, dd = _anchored(s)
        cols = np.flatnonzero((dd == value).any(axis=0))
        if len(cols):
            c = int(cols[0])
            r = int(np.flatnonzero(dd[:, c] == value)[0])
            i0, j0 = i1 - r, j1 - c
            break
        assert lo > 0, "no alignment of the value ends in the end cell"
        width *= 4
    s = prof[t[j0:j1 + 1]][:, i0:i1 + 1].T
    ha, ea, fa, dd = _anchored(s)
    assert int(ha[-1, -1]) == value
    runs = _traceback(ha, ea, fa, dd)
    return i0, i1, j0, j1, "".join(f"{n}{o}" for n, o in runs)


def rescore(rna: bytes, target: bytes, i0: int, j0: int, cigar: str):
    """Score of a CIGAR over the unit's target codes from the cell (i0, j0), and the cell of its last pair."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = _CODE[np.frombuffer(target, dtype=np.uint8)]
    i, j, score = i0, j0, 0
    for n, o in re.findall(r"(\d+)([MID])", cigar):
        n = int(n)
        if o == "M":
            for k in range(n):
                score += 5 if (q[i + k] == t[j + k] and t[j + k] < 4) else -4
            i, j = i + n, j + n
        else:
            score -= 16 + 4 * (n - 1)
            if o == "I":
                i += n
            else:
                j += n
    return score, i - 1, j - 1


def enc_info(enc: int):
    """(strand, para, rule) of an encoding."""
    if enc < 12:
        return enc & 1, 1, enc // 2 + 1
    return (0 if (enc - 12) & 1 else 1), -1, (enc - 12) // 2 + 1


_STAB = {1: {"AT": 3.7, "TG": 2.8, "GG": 2.2, "GT": 2.4, "GC": 4.5, "CT": 2.6, "CC": 2.4},
         -1: {"AA": 3.0, "AT": 3.5, "AC": 1.0, "TG": 1.0, "GA": 1.0, "GG": 3.0, "GC": 3.0, "CT": 2.0, "CC": 1.0}}


def triplex_record(rna: bytes, seg: bytes, enc: int, a_s: int, value: int, i0, i1, j0, j1, cigar: str, p):
    """convertMyTriplex's numbers and strings for one alignment of a unit, ntMin = 1 and no ntMax.  The TTS strand of the
    strand-1 encodings is complement(), which drops every letter outside ACGTN (so later letters move up, and the string ends
    where that strand runs out); the other encodings show the segment's letters as they are."""
    n = len(seg)
    strand, para, rule = enc_info(enc)
    target = encode_unit(seg, enc).decode()
    if strand == 1:
        src = bytes(c for c in seg if c in b"ACGTN").translate(bytes.maketrans(b"ACGT", b"TGCA"))
    else:
        src = seg
    src = (src[::-1] if enc & 1 else src).decode() + "\0" * n
    tgt, tts, tfo = [], [], []
    q, r = j0, i0
    for cnt, o in re.findall(r"(\d+)([MID])", cigar):
        for _ in range(int(cnt)):
            if o == "I":
                tgt.append("-"); tts.append("-"); tfo.append(chr(rna[r])); r += 1
            else:
                tgt.append(target[q]); tts.append(src[q]); q += 1
                if o == "D":
                    tfo.append("-")
                else:
                    tfo.append(chr(rna[r])); r += 1
    nt = len(tgt)
    match = sum(1 for x, y in zip(tgt, tfo) if x == y)
    identity = np.float32(100 * match) / np.float32(nt)
    tri = np.float32(0)
    prev_v, prev_c = np.float32(0), ""
    pt, pc = np.float32(p.penaltyT), np.float32(p.penaltyC)
    for k in range(nt):
        cur = "-" if tgt[k] == "-" else tts[k]
        v = np.float32(_STAB[para].get(cur + tfo[k], 0.0))
        if cur == prev_c and cur == "T":
            tri = np.float32(np.float32(tri - prev_v) + pt); v = pt
        if cur == prev_c and cur == "C":
            tri = np.float32(np.float32(tri - prev_v) + pc); v = pc
        prev_v = v
        if tgt[k] != "-":
            prev_c = cur
        tri = np.float32(tri + v)
    tri = np.float32(tri / np.float32(nt))
    if enc & 1:
        rs, re_ = n - j1 - 1, n - j0 - 1
    else:
        rs, re_ = j0 + 1, j1 + 1
    return dict(stari=i0 + 1, endi=i1 + 1, starj=rs + a_s, endj=re_ + a_s, strand=strand, reverse=para, rule=rule, nt=nt,
                score=np.float32(value), identity=np.float32(identity), tri_score=tri, enc=enc, tfo="".join(tfo),
                tts="".join(tts).split("\0")[0])


def site_hits(rna: bytes, dna: bytes, p, sites, seg_first=0, seg_count=-1):
    """The hits of a record's sites ((n, 6) rows of cls, start, end, value, pos, enc): per site a dict with seg, enc, i0, i1, j0,
    j1, jp, n, cigar and the triplex record.  One unit's matrix is computed once and serves all the sites of that unit."""
    step = p.cutLength - p.overlapLength
    starts = list(range(0, len(dna), step))
    last = len(starts) if seg_count < 0 else min(len(starts), seg_first + seg_count)
    cache = {}
    order = sorted(range(len(sites)), key=lambda k: (int(sites[k][4]) // step, int(sites[k][5])))
    out = [None] * len(sites)
    for k in order:
        cls, start, end, value, pos, enc = (int(x) for x in sites[k])
        found = None
        for s in range(max(0, seg_first), last):
            a = starts[s]
            seg = dna[a:a + p.cutLength]
            if not (a <= pos < a + len(seg)) or same_seq(seg):
                continue
            if (s, enc) not in cache:
                if len(cache) >= 3:
                    cache.pop(next(iter(cache)))
                cache[(s, enc)] = unit_matrix(rna, encode_unit(seg, enc))
            H = cache[(s, enc)]
            jp = len(seg) - 1 - (pos - a) if enc & 1 else pos - a
            if int(H[:, jp].max()) == value:
                found = (s, a, seg, H, jp)
                break
        assert found is not None, (k, sites[k])
        s, a, seg, H, jp = found
        i0, i1, j0, j1, cigar = align_in_unit(rna, encode_unit(seg, enc), H, jp, value)
        rec = triplex_record(rna, seg, enc, a, value, i0, i1, j0, j1, cigar, p)
        rec["seg"] = s
        out[k] = dict(seg=s, enc=enc, i0=i0, i1=i1, j0=j0, j1=j1, jp=jp, n=len(seg), cigar=cigar, rec=rec)
    return out


def site_hit(rna: bytes, dna: bytes, p, site, seg_first=0, seg_count=-1):
    return site_hits(rna, dna, p, [site], seg_first, seg_count)[0]


def hits_array(hits):
    """(n, 8) int64 rows of seg, enc, i0, i1, j0, j1, nt, cigar_len: what SiteHits.array() returns."""
    return np.asarray([(h["seg"], h["enc"], h["i0"], h["i1"], h["j0"], h["j1"], h["rec"]["nt"], len(re.findall(r"[MID]", h["cigar"])))
                       for h in hits], dtype=np.int64).reshape(-1, 8)


# ---- a scalar triple-matrix implementation of the same definition ----------------------------------------------------------------
def _score(qc, tc):
    return 5 if (qc == tc and tc < 4) else -4


def scalar_hit(rna: bytes, target: bytes, jp: int, value: int):
    q = [int(_CODE[c]) for c in rna]
    t = [int(_CODE[c]) for c in target]
    m, n = len(q), len(t)
    rows = 16 * ((m + 15) // 16)
    H = [[0] * n for _ in range(rows)]
    E = [[0] * n for _ in range(rows)]
    for j in range(n):
        f = 0
        for i in range(rows):
            s = 0 if i >= m else _score(q[i], t[j])
            e = max(E[i][j - 1] - 4, H[i][j - 1] - 16, 0) if j else 0
            f = max(f - 4, H[i - 1][j] - 16, 0) if i else 0
            d = (H[i - 1][j - 1] if i and j else 0) + s
            H[i][j] = max(0, d, e, f)
            E[i][j] = e
    assert max(H[i][jp] for i in range(rows)) == value
    j1 = max(j for j in range(jp + 1) if any(H[i][j] == value for i in range(m)))
    i1 = min(i for i in range(m) if H[i][j1] == value)
    # G by three matrices on the reversed rectangle, all of it
    R, C = i1 + 1, j1 + 1
    Hr = [[NEG] * C for _ in range(R)]
    Er = [[NEG] * C for _ in range(R)]
    Fr = [[NEG] * C for _ in range(R)]
    G = [[NEG] * C for _ in range(R)]
    for c in range(C):
        for r in range(R):
            s = _score(q[i1 - r], t[j1 - c])
            d = (0 if (r == 0 and c == 0) else (Hr[r - 1][c - 1] if r and c else NEG)) + s
            e = max(Er[r][c - 1] - 4, Hr[r][c - 1] - 16) if c else NEG
            f = max(Fr[r - 1][c] - 4, Hr[r - 1][c] - 16) if r else NEG
            G[r][c], Er[r][c], Fr[r][c] = d, max(e, NEG), max(f, NEG)
            Hr[r][c] = max(d, e, f, NEG)
    c0 = min(c for c in range(C) if any(G[r][c] == value for r in range(R)))
    r0 = min(r for r in range(R) if G[r][c0] == value)
    i0, j0 = i1 - r0, j1 - c0
    R, C = i1 - i0 + 1, j1 - j0 + 1
    Ha = [[NEG] * C for _ in range(R)]
    Ea = [[NEG] * C for _ in range(R)]
    Fa = [[NEG] * C for _ in range(R)]
    Da = [[NEG] * C for _ in range(R)]
    for c in range(C):
        for r in range(R):
            s = _score(q[i0 + r], t[j0 + c])
            d = (0 if (r == 0 and c == 0) else (Ha[r - 1][c - 1] if r and c else NEG)) + s
            e = max(Ea[r][c - 1] - 4, Ha[r][c - 1] - 16) if c else NEG
            f = max(Fa[r - 1][c] - 4, Ha[r - 1][c] - 16) if r else NEG
            Da[r][c], Ea[r][c], Fa[r][c] = max(d, NEG), max(e, NEG), max(f, NEG)
            Ha[r][c] = max(d, e, f, NEG)
    # the traceback of the definition, written out again over the scalar lists: in H the diagonal first, then E, then F; in a
    # gap state extension first, then opening
    r, c, state, path = R - 1, C - 1, 0, ""
    while True:
        s = _score(q[i0 + r], t[j0 + c])
        if state == 0:
            prev = 0 if (r == 0 and c == 0) else (Ha[r - 1][c - 1] if r and c else NEG)
            if Ha[r][c] == prev + s:
                path += "M"
                if r == 0 and c == 0:
                    break
                r, c = r - 1, c - 1
            elif Ha[r][c] == Ea[r][c]:
                state = 1
            else:
                state = 2
        elif state == 1:
            path += "D"
            state = 1 if Ea[r][c] == Ea[r][c - 1] - 4 else 0
            c -= 1
        else:
            path += "I"
            state = 2 if Fa[r][c] == Fa[r - 1][c] - 4 else 0
            r -= 1
    cigar = "".join(f"{len(x.group(0))}{x.group(0)[0]}" for x in re.finditer(r"M+|I+|D+", path[::-1]))
    return i0, i1, j0, j1, cigar


def _planted(rng, m, n, kind, at_end=False):
    """A random query and target with one gapped copy of a query stretch planted in the target (at_end: the query's last 30
    bases, so that the pad rows echo the hit into the columns after it)."""
    q = rng.choice(list(b"ACGT"), size=m).astype(np.uint8).tobytes()
    t = bytearray(rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes())
    a = m - 30 if at_end else int(rng.integers(0, m - 30))
    piece = q[a:a + 30]
    if kind == 1:
        piece = piece[:14] + piece[16:]                 # two query bases against a gap: I
    elif kind == 2:
        piece = piece[:15] + b"TT" + piece[15:]         # two target bases against a gap: D
    at = int(rng.integers(0, n - len(piece)))
    t[at:at + len(piece)] = piece
    return q, bytes(t)


def test_restatement_equals_the_scalar_matrices():
    rng = np.random.default_rng(15)
    seen_i = seen_d = seen_echo = 0
    for trial in range(12):
        q, t = _planted(rng, 40, 120, trial % 3, at_end=trial % 4 == 3)
        H = unit_matrix(q, t)
        cm = H.max(axis=0)
        value = int(cm.max())
        for jp in sorted({int(np.argmax(cm)), int(np.flatnonzero(cm == value)[-1])}):
            v = int(cm[jp])
            got = align_in_unit(q, t, H, jp, v)
            want = scalar_hit(q, t, jp, v)
            assert got == want, (trial, jp, got, want)
            sc, ie, je = rescore(q, t, got[0], got[2], got[4])
            assert (sc, ie, je) == (v, got[1], got[3])
            assert got[4][-1] == "M" and re.match(r"\d+M", got[4])
            seen_i += "I" in got[4]
            seen_d += "D" in got[4]
            seen_echo += got[3] < jp
    assert seen_i >= 1 and seen_d >= 1 and seen_echo >= 1


@pytest.fixture(scope="module")
def demo(golden_dir):
    rna = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    dna = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    return rna, dna


def test_rescoring_the_cigar_gives_the_value_on_the_demo(mod, demo):
    """Consequence (a) on every hit of the demo at V = int(0.8 x top)."""
    rna, dna = demo
    p = mod.default_params()
    P, per_enc = expected_potential(rna, dna, p)
    v = int(0.8 * int(P.max()))
    sites = sites_from(P, per_enc, v)
    assert len(sites) >= 4
    hits = site_hits(rna, dna, p, sites)
    for site, h in zip(sites.tolist(), hits):
        seg = dna[:p.cutLength]
        sc, ie, je = rescore(rna, encode_unit(seg, h["enc"]), h["i0"], h["j0"], h["cigar"])
        assert (sc, ie, je) == (site[3], h["i1"], h["j1"]), (site, h["cigar"])
        assert h["jp"] - h["j1"] <= 15 and (h["enc"] & 1 or h["jp"] == h["j1"])
        assert h["rec"]["nt"] == sum(int(n) for n in re.findall(r"(\d+)[MID]", h["cigar"]))
        assert h["rec"]["stari"] == h["i0"] + 1 and h["rec"]["endi"] == h["i1"] + 1


def _tie_to_ssw_align(orc, rna, targets, what):
    """Where the reference's column maxima stay below 148: the hit of the unit's best cell has the score ssw_align returns, and
    rescore() applied to the oracle's own CIGAR and begin cells returns that score too (which validates the helper)."""
    compared = left_out = 0
    for k, t in enumerate(targets):
        if max(orc.pre_align(rna, t)) >= 148:
            left_out += 1
            continue
        (sw_score, ref_begin, ref_end, query_begin, query_end), cigar = orc.align(rna, t)
        H = unit_matrix(rna, t)
        cm = H.max(axis=0)
        value = int(cm.max())
        assert value == sw_score, (what, k, value, sw_score)
        compared += 1
        if sw_score == 0:
            continue
        sc, ie, je = rescore(rna, t, query_begin, ref_begin, cigar)
        assert (sc, ie, je) == (sw_score, query_end, ref_end), (what, k, cigar)
        i0, i1, j0, j1, cg = align_in_unit(rna, t, H, int(np.argmax(cm)), value)
        assert rescore(rna, t, i0, j0, cg) == (sw_score, i1, j1), (what, k, cg)
    return compared, left_out


def test_hit_of_the_best_cell_equals_ssw_align_below_148(oracle_build, golden_dir, demo):
    orc = helpers.Oracle(oracle_build)
    h19, dna = demo
    assert len(dna) <= 5000
    compared, left_out = _tie_to_ssw_align(orc, h19, [orc.encode_unit(dna, e)[0] for e in range(48)], "demo")
    print(f"demo: {compared} units compared, {left_out} left out")
    assert compared + left_out == 48 and compared >= 20
    meg3 = synth.read_fasta(os.path.join(golden_dir, "MEG3.fa"))[1]
    compared = left_out = 0
    for k, (_, rec) in enumerate(helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:6]):
        c, o = _tie_to_ssw_align(orc, meg3, [orc.encode_unit(rec[:5000], e)[0] for e in range(48)], f"peak {k}")
        compared, left_out = compared + c, left_out + o
    print(f"MEG3 peaks: {compared} units compared, {left_out} left out")
    assert compared + left_out == 6 * 48
    assert left_out <= 0.05 * (compared + left_out)


# ---- the host functions of the library ---------------------------------------------------------------------------------------------
def _hand_made(mod):
    """Two shards of one record as the library would return them, built through the C structures."""
    import ctypes as C
    keep = []

    def hits(rows):
        n = len(rows)
        h = mod._SiteHits()
        t = (mod.Triplex * max(1, n))()
        qb, qe, tb, te = ((C.c_int32 * max(1, n))() for _ in range(4))
        off = (C.c_int64 * max(1, n))()
        ln = (C.c_int32 * max(1, n))()
        cig, pool = [], bytearray(b"\0")
        for k, r in enumerate(rows):
            t[k].seg, t[k].enc, t[k].stari, t[k].endi, t[k].starj, t[k].endj = r["seg"], r["enc"], r["stari"], r["endi"], r["starj"], r["endj"]
            t[k].rule, t[k].nt, t[k].identity, t[k].tri_score, t[k].score = r["rule"], r["nt"], r["identity"], r["tri"], r["score"]
            qb[k], qe[k], tb[k], te[k] = r["cells"]
            off[k] = len(cig)
            if r["cigar"] is None:
                ln[k] = -1
                continue
            ln[k] = len(r["cigar"])
            cig += r["cigar"]
            t[k].tfo_off = len(pool); pool += r["tfo"].encode() + b"\0"
            t[k].tts_off = len(pool); pool += r["tts"].encode() + b"\0"
        cg = (C.c_uint32 * max(1, len(cig)))(*cig)
        pl = C.create_string_buffer(bytes(pool), len(pool))
        h.n, h.t, h.q_begin, h.q_end, h.t_begin, h.t_end = n, t, qb, qe, tb, te
        h.cigar_off, h.cigar_len, h.cigar, h.pool, h.pool_len = off, ln, cg, C.cast(pl, C.POINTER(C.c_char)), len(pool)
        h.unaligned = sum(1 for r in rows if r["cigar"] is None)
        keep.append((t, qb, qe, tb, te, off, ln, cg, pl, h))
        return mod.SiteHits(C.pointer(h), _keep=keep[-1])

    return hits, keep


def _row(seg, enc, cigar, **kw):
    d = dict(seg=seg, enc=enc, stari=3, endi=12, starj=101, endj=110, rule=1, nt=10, identity=90.0, tri=1.25, score=41.0,
             cells=(2, 11, 100, 109), cigar=cigar, tfo="ACGUACGUAC", tts="ACGTACGTAC")
    d.update(kw)
    return d


def test_site_hits_tsv_bytes(mod):
    make, keep = _hand_made(mod)
    sites = mod.Sites([(0, 100, 112, 41, 109, 0), (1, 300, 305, 30, 302, 1), (2, 400, 401, 16383, 400, 12)], min_value=30, max_gap=2)
    h = make([_row(0, 0, [(10 << 4)]),
              _row(0, 1, [(4 << 4), (2 << 4) | 1, (3 << 4), (1 << 4) | 2, (2 << 4)], starj=295, endj=304, nt=12, identity=75.0, tri=0.5,
                   tfo="ACGUAC-GUACG", tts="ACGT--CGTACG"),
              _row(-1, 12, None)])
    got = mod.site_hits_tsv(sites, h, "chr7", 1001, "toy")
    want = (b"# fasim site hits lncRNA=toy min_value=30 max_gap=2\n"
            b"chrom\ttts_start\ttts_end\tclass\tvalue\tstrand\trule\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tTFO\tTTS\n"
            b"chr7\t1100\t1110\tParaPlus\t41\t+\t1\t3\t12\t10\t90\t1.25\t10M\tACGUACGUAC\tACGTACGTAC\n"
            b"chr7\t1295\t1305\tParaMinus\t30\t-\t1\t3\t12\t12\t75\t0.5\t4M2I3M1D2M\tACGUAC-GUACG\tACGT--CGTACG\n"
            b"chr7\t1400\t1401\tAntiMinus\t16383\t-\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n")
    assert got == want
    named = mod.site_hits_tsv(sites, h, "chr7", 1001, "toy", record_name="peak_1", header=False)
    assert named == b"".join(line + b"\tpeak_1\n" for line in want.split(b"\n")[2:-1])
    with pytest.raises(mod.FasimError) as ei:
        mod.site_hits_tsv(mod.Sites([(0, 1, 2, 30, 1, 0)], min_value=30), h, "chr7", 1, "toy")
    assert ei.value.code == mod.E_ARG
    del h


def test_site_hits_merge_tie_rules_and_refusals(mod):
    make, keep = _hand_made(mod)
    # shard A: segments 0-1, shard B: segments 2-3.  Class 0: the same peak seen by both (a full tie: the smaller seg wins) inside
    # intervals that unite; class 1: B's site has the larger value; class 2: only A has it, unaligned
    sa = mod.Sites([(0, 100, 112, 41, 109, 0), (1, 300, 305, 30, 302, 1), (2, 900, 901, 16383, 900, 12)], min_value=30, units=4, raw_runs=3)
    sb = mod.Sites([(0, 110, 120, 41, 109, 0), (1, 305, 309, 35, 306, 3)], min_value=30, units=4, raw_runs=2)
    ha = make([_row(1, 0, [(10 << 4)]), _row(1, 1, [(9 << 4)], nt=9), _row(-1, 12, None)])
    hb = make([_row(2, 0, [(10 << 4)], tfo="GGGGGGGGGG"), _row(2, 3, [(7 << 4)], nt=7, tfo="CCCCCCC", tts="GGGGGGG")])
    for order in ((sa, ha, sb, hb), (sb, hb, sa, ha)):
        s, h = mod.merge_site_hits([order[0], order[2]], [order[1], order[3]])
        assert s.array().tolist() == [[0, 100, 120, 41, 109, 0], [1, 300, 309, 35, 306, 3], [2, 900, 901, 16383, 900, 12]]
        assert np.array_equal(s.array(), mod.merge_sites([sa, sb]).array())
        assert h.array().tolist() == [[1, 0, 2, 11, 100, 109, 10, 1], [2, 3, 2, 11, 100, 109, 7, 1], [-1, 12, 2, 11, 100, 109, 10, -1]]
        assert h.cigars() == ["10M", "7M", ""] and h.unaligned == 1
        tr = h.triplexes()
        assert tr[0]["tfo"] == "ACGUACGUAC" and tr[1]["tfo"] == "CCCCCCC" and tr[1]["tts"] == "GGGGGGG" and tr[2]["tfo"] == ""
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_hits([sa, sb], [ha, ha])                    # hits that do not belong to the sites
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_hits([sa, mod.Sites([(0, 1, 2, 40, 1, 0)], min_value=40)], [ha, make([_row(0, 0, [16])])])
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_hits([], [])
    assert ei.value.code == mod.E_ARG
    del ha, hb


def test_site_hits_symbols_are_exported(mod):
    for s in ("fasim_scan_records_sites_aligned", "fasim_site_hits_merge", "fasim_site_hits_tsv", "fasim_site_hits_free"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    for s in ("SiteHits", "merge_site_hits", "site_hits_tsv"):
        assert hasattr(mod, s)
    assert hasattr(mod.Engine, "scan_sites_aligned")


@pytest.mark.parametrize("extra", [[], ["-F"], ["--track", "25"]])
def test_cli_refuses_sites_align_without_sites(mod, tmp_path, golden_dir, extra):
    """--sites-align is valid only with --sites V (and what --sites refuses stays refused): status 2, nothing written."""
    exe = os.path.join(entry.PKG_DIR, "fasim")
    args = [exe, "-f1", os.path.join(golden_dir, "testDNA.fa"), "-f2", os.path.join(golden_dir, "H19.fa"), "-O", str(tmp_path), "--sites-align"]
    if extra:
        args += ["--sites", "100"] + extra
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2, r.stderr
    assert os.listdir(tmp_path) == []
