"""Potential tracks (fasim_scan_track), the part that needs no GPU: the yardstick of the GPU tests -- an independent numpy
restatement of the definition in DESIGN.md section 11, tied here to the oracle's restatement of the reference -- and the two pure
host functions of the C-ABI, fasim_track_merge and fasim_track_bedgraph.

The restatement never calls the code under test.  Per unit (segment x encoding) it is the textbook Gotoh local alignment of the
lncRNA against the unit's target, column by column over all rows at once:
    H' = max(0, Hdiag + s, E)
    F[i] = max over k < i of (H'[k] + 4 k) - 4 i - 12        (a gap of i - k residues from row k: 16 + 4 (i - k - 1))
    H = max(H', F)                                            (exact: a cell reached by a gap never opens a better gap than
    E = max(E - 4, H - 16, 0)                                  the one it came by)
with the stage-2 scoring (+5 / -4 over ACGT, every other letter -4, query U read as A) and the reference's zero-score pad rows up
to 16 * ceil(m / 16).  No overflow cut, no lazy-F deviation."""
import os

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry

CLASS_NAMES = ("ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus")
_CODE = np.full(256, 4, dtype=np.int64)
for _letters, _c in (("AaUu", 0), ("Cc", 1), ("Gg", 2), ("Tt", 3)):
    for _ch in _letters:
        _CODE[ord(_ch)] = _c


def colmax_units(rna: bytes, targets):
    """Column maxima of the definition for several targets of one length: (len(targets), n) int64."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    m = len(q)
    rows = 16 * ((m + 15) // 16)
    t = np.stack([_CODE[np.frombuffer(x, dtype=np.uint8)] for x in targets])          # (units, n)
    nu, n = t.shape
    # score of target code c against every row: prof[c] (pad rows 0)
    prof = np.zeros((5, rows), dtype=np.int64)
    for c in range(5):
        prof[c, :m] = np.where((q == c) & (q < 4), 5, -4)
    ramp = 4 * np.arange(rows, dtype=np.int64)
    h = np.zeros((nu, rows), dtype=np.int64)
    e = np.zeros((nu, rows), dtype=np.int64)
    out = np.zeros((nu, n), dtype=np.int64)
    diag = np.zeros((nu, rows), dtype=np.int64)
    for j in range(n):
        diag[:, 1:] = h[:, :-1]
        hp = np.maximum(np.maximum(diag + prof[t[:, j]], e), 0)
        run = np.maximum.accumulate(hp + ramp, axis=1)
        f = np.zeros_like(hp)
        f[:, 1:] = run[:, :-1] - ramp[1:] - 12
        h = np.maximum(hp, f)
        e = np.maximum(np.maximum(e - 4, h - 16), 0)
        out[:, j] = h.max(axis=1)
    return out


def colmax_scalar(rna: bytes, target: bytes):
    """The same as a plain double loop with explicit E and F (for a spot check of the vectorised form)."""
    q = [int(_CODE[c]) for c in rna]
    rows = 16 * ((len(q) + 15) // 16)
    h_prev, e_prev = [0] * (rows + 1), [0] * (rows + 1)
    out = []
    for ch in target:
        tc = int(_CODE[ch])
        h, e = [0] * (rows + 1), [0] * (rows + 1)
        f, best = 0, 0
        for i in range(1, rows + 1):
            s = 0 if i > len(q) else (5 if (q[i - 1] == tc and tc < 4) else -4)
            e[i] = max(e_prev[i] - 4, h_prev[i] - 16, 0)
            f = max(f - 4, h[i - 1] - 16, 0)
            h[i] = max(0, h_prev[i - 1] + s, e[i], f)
            best = max(best, h[i])
        out.append(best)
        h_prev, e_prev = h, e
    return out


def enabled_encodings(p):
    v = []
    if p.strand >= 0:
        v += list(range(12)) if p.rule == 0 else ([2 * (p.rule - 1), 2 * (p.rule - 1) + 1] if 0 < p.rule < 7 else [])
    if p.strand <= 0:
        v += list(range(12, 48)) if p.rule == 0 else ([12 + 2 * (p.rule - 1), 12 + 2 * (p.rule - 1) + 1] if 1 <= p.rule <= 18 else [])
    return v


def enc_class(enc: int) -> int:
    """0 ParaPlus (para 1, strand 0), 1 ParaMinus (1, 1), 2 AntiMinus (-1, 1), 3 AntiPlus (-1, 0)."""
    if enc < 12:
        return enc & 1
    return 3 if (enc - 12) & 1 else 2


def encode_unit(seg: bytes, enc: int) -> bytes:
    """Target letters of the unit: the rule's output for A, T, G, C, N for every other letter (lower case too), reversed for the
    odd encodings."""
    table = bytearray(b"N" * 256)
    for base, o in zip(b"ATGC", synth.RULE_OUT[enc].encode()):
        table[base] = o
    t = seg.translate(bytes(table))
    return t[::-1] if enc & 1 else t


def same_seq(seg: bytes) -> bool:
    return len(seg) == 0 or (seg[:1] in (b"A", b"C", b"G", b"T", b"U", b"N") and seg == seg[:1] * len(seg))


def expected_tracks(rna: bytes, dna: bytes, p, seg_first=0, seg_count=-1, colmax=None):
    """P[c][x] of the definition, (4, len(dna)) int64, and per class the largest column maximum of its units.  `colmax(rna,
    targets)` gives the column maxima of equally long targets (default: the restatement)."""
    colmax = colmax or colmax_units
    big = len(dna)
    step = p.cutLength - p.overlapLength
    starts = list(range(0, big, step))
    last = len(starts) if seg_count < 0 else min(len(starts), seg_first + seg_count)
    encs = enabled_encodings(p)
    out = np.zeros((4, big), dtype=np.int64)
    top = [0, 0, 0, 0]
    for a in starts[seg_first:last]:
        seg = dna[a:a + p.cutLength]
        if same_seq(seg):
            continue
        cm = np.asarray(colmax(rna, [encode_unit(seg, e) for e in encs]))
        for k, e in enumerate(encs):
            c = enc_class(e)
            row = cm[k][::-1] if e & 1 else cm[k]
            out[c, a:a + len(seg)] = np.maximum(out[c, a:a + len(seg)], row)
            top[c] = max(top[c], int(row.max()))
    return out, top


def bin_reduce(a, width: int):
    """track[c][b] = max of P[c][x] over x in [b * width, (b + 1) * width)."""
    n = a.shape[1]
    nb = (n + width - 1) // width
    pad = np.zeros((a.shape[0], nb * width), dtype=a.dtype)
    pad[:, :n] = a
    return pad.reshape(a.shape[0], nb, width).max(axis=2)


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def test_restatement_equals_the_oracle_below_148(oracle_build, golden_dir):
    """Every unit of the demo (testDNA.fa x H19.fa, one segment, 48 encodings) whose reference column maxima all stay below 148
    (no F can reach 132, no column 251: Q1 and Q2 cannot show) must give the same maxima in the restatement.  26 of the 48
    units qualify.  Also ties the test's own unit encoding to the oracle's, and the vectorised form to a scalar double loop."""
    orc = helpers.Oracle(oracle_build)
    rna = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    dna = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    assert len(dna) <= 5000
    targets = [orc.encode_unit(dna, e)[0] for e in range(48)]
    assert targets == [encode_unit(dna, e) for e in range(48)]
    mine = colmax_units(rna, targets)
    compared = 0
    for e in range(48):
        ref = orc.pre_align(rna, targets[e])
        if max(ref) >= 148:
            continue
        compared += 1
        assert mine[e].tolist() == ref, f"encoding {e}"
    print(f"{compared} of 48 units compared")
    assert compared >= 20
    # a unit the reference cuts off, against the scalar double loop (first 600 columns: the double loop is slow)
    hot = max(range(48), key=lambda e: int(mine[e].max()))
    assert int(mine[hot].max()) > 250
    assert colmax_units(rna, [targets[hot][:600]])[0].tolist() == colmax_scalar(rna, targets[hot][:600])


def test_restatement_classes_and_bins():
    assert [enc_class(e) for e in (0, 1, 12, 13, 46, 47)] == [0, 1, 2, 3, 2, 3]
    a = np.arange(14, dtype=np.int64).reshape(2, 7)
    assert bin_reduce(a, 3).tolist() == [[2, 5, 6], [9, 12, 13]]
    assert bin_reduce(a, 1).tolist() == a.tolist()


def test_track_merge_is_the_maximum(mod):
    rng = np.random.default_rng(5)
    parts = [rng.integers(0, 16384, size=(4, 37)).astype(np.uint16) for _ in range(3)]
    tracks = [mod.Track(a, bin=25, units=k + 1, saturated_units=k) for k, a in enumerate(parts)]
    got = mod.merge_tracks(tracks)
    assert (got.bin, got.nbins, got.units, got.saturated_units) == (25, 37, 6, 3)
    arr = got.array()
    assert arr.dtype == np.uint16 and arr.shape == (4, 37)
    assert np.array_equal(arr, np.maximum(np.maximum(parts[0], parts[1]), parts[2]))
    assert np.array_equal(mod.merge_tracks(tracks[:1]).array(), parts[0])
    for other in (mod.Track(parts[1], bin=24), mod.Track(parts[1][:, :36], bin=25)):
        with pytest.raises(mod.FasimError) as ei:
            mod.merge_tracks([tracks[0], other])
        assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_tracks([])
    assert ei.value.code == mod.E_ARG


def test_track_bedgraph_bytes(mod):
    """Runs of equal neighbouring bins are joined, bins below min_value and zeros are absent, the last bin is clipped to the
    record length, coordinates are 0-based half-open genome positions (start_genome = 1-based position of the first base), and
    the four blocks come in class order."""
    v = np.zeros((4, 10), dtype=np.uint16)
    v[0, 2:5] = 7
    v[0, 5] = 9
    v[0, 7] = 2
    v[1, 0] = 1
    v[3, 8:10] = 300
    t = mod.Track(v, bin=25)
    head = "track type=bedGraph name='H19 potential (%s)'\n"
    want = (head % "ParaPlus" + "chr11\t1050\t1125\t7\nchr11\t1125\t1150\t9\nchr11\t1175\t1200\t2\n" +
            head % "ParaMinus" + "chr11\t1000\t1025\t1\n" +
            head % "AntiMinus" +
            head % "AntiPlus" + "chr11\t1200\t1240\t300\n")
    assert mod.track_bedgraph(t, "chr11", 1001, 240, "H19") == want.encode()
    want3 = (head % "ParaPlus" + "chr11\t1050\t1125\t7\nchr11\t1125\t1150\t9\n" + head % "ParaMinus" + head % "AntiMinus" +
             head % "AntiPlus" + "chr11\t1200\t1240\t300\n")
    assert mod.track_bedgraph(t, "chr11", 1001, 240, "H19", min_value=3) == want3.encode()
    # bin = 1, genome start 1: position x is [x, x + 1)
    one = np.zeros((4, 5), dtype=np.uint16)
    one[2] = [4, 4, 0, 5, 4]
    got = mod.track_bedgraph(mod.Track(one, bin=1), "c", 1, 5, "q")
    assert got == ("track type=bedGraph name='q potential (ParaPlus)'\ntrack type=bedGraph name='q potential (ParaMinus)'\n"
                   "track type=bedGraph name='q potential (AntiMinus)'\nc\t0\t2\t4\nc\t3\t4\t5\nc\t4\t5\t4\n"
                   "track type=bedGraph name='q potential (AntiPlus)'\n").encode()
    for bad in (dict(dna_len=251), dict(dna_len=225), dict(min_value=0)):
        kw = dict(dna_len=240, min_value=1)
        kw.update(bad)
        with pytest.raises(mod.FasimError) as ei:
            mod.track_bedgraph(t, "chr11", 1001, kw["dna_len"], "H19", kw["min_value"])
        assert ei.value.code == mod.E_ARG


def test_track_symbols_are_exported(mod):
    for s in ("fasim_scan_track", "fasim_track_merge", "fasim_track_bedgraph", "fasim_track_free"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
