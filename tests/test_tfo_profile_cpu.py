"""Per-base profile of the lncRNA (fasim_scan_tfo_profile), the part that needs no GPU: the yardstick of the GPU tests -- the numpy
restatement of test_track_cpu.py with one more running maximum, per ROW instead of per column -- tied here to
the reference's own ssw_align through the oracle, and the two pure host functions of the C-ABI, fasim_tfo_profile_merge and
fasim_tfo_profile_tsv.

The restatement never calls the code under test.  R_unit[i] = max over the real columns j of H[i][j], rows [0, m) only."""
import os

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, colmax_units, enabled_encodings, enc_class, encode_unit, same_seq

HEADER = b"pos\tbase\tParaPlus\tParaMinus\tAntiMinus\tAntiPlus\n"


def rowmax_units(rna: bytes, targets):
    """(column maxima (units, n), row maxima (units, m)) of the definition for several targets of one length: the loop of
    test_track_cpu.colmax_units with `rm = maximum(rm, h)` per column."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    m = len(q)
    rows = 16 * ((m + 15) // 16)
    t = np.stack([_CODE[np.frombuffer(x, dtype=np.uint8)] for x in targets])          # (units, n)
    nu, n = t.shape
    prof = np.zeros((5, rows), dtype=np.int64)
    for c in range(5):
        prof[c, :m] = np.where((q == c) & (q < 4), 5, -4)
    ramp = 4 * np.arange(rows, dtype=np.int64)
    h = np.zeros((nu, rows), dtype=np.int64)
    e = np.zeros((nu, rows), dtype=np.int64)
    cm = np.zeros((nu, n), dtype=np.int64)
    rm = np.zeros((nu, rows), dtype=np.int64)
    diag = np.zeros((nu, rows), dtype=np.int64)
    for j in range(n):
        diag[:, 1:] = h[:, :-1]
        hp = np.maximum(np.maximum(diag + prof[t[:, j]], e), 0)
        run = np.maximum.accumulate(hp + ramp, axis=1)
        f = np.zeros_like(hp)
        f[:, 1:] = run[:, :-1] - ramp[1:] - 12
        h = np.maximum(hp, f)
        e = np.maximum(np.maximum(e - 4, h - 16), 0)
        cm[:, j] = h.max(axis=1)
        rm = np.maximum(rm, h)
    return cm, rm[:, :m]


def rowmax_scalar(rna: bytes, target: bytes):
    """The same as a plain double loop with explicit E and F: (column maxima, row maxima over rows [0, m))."""
    q = [int(_CODE[c]) for c in rna]
    rows = 16 * ((len(q) + 15) // 16)
    h_prev, e_prev = [0] * (rows + 1), [0] * (rows + 1)
    cols, rmax = [], [0] * (rows + 1)
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
            rmax[i] = max(rmax[i], h[i])
        cols.append(best)
        h_prev, e_prev = h, e
    return cols, rmax[1:len(q) + 1]


def expected_profiles(rna: bytes, records, p, seg_first=0, seg_count=-1):
    """R[c][i] of the definition per record: a list of (4, m) int64 arrays, and the number of units that contributed.  Segments are
    numbered globally, record after record; only [seg_first, seg_first + seg_count) contribute."""
    step = p.cutLength - p.overlapLength
    encs = enabled_encodings(p)
    out, units, g = [], 0, 0
    for dna in records:
        prof = np.zeros((4, len(rna)), dtype=np.int64)
        for a in range(0, len(dna), step):
            g += 1
            if g - 1 < seg_first or (seg_count >= 0 and g - 1 >= seg_first + seg_count):
                continue
            seg = dna[a:a + p.cutLength]
            if same_seq(seg):
                continue
            _, rm = rowmax_units(rna, [encode_unit(seg, e) for e in encs])
            for k, e in enumerate(encs):
                c = enc_class(e)
                prof[c] = np.maximum(prof[c], rm[k])
            units += len(encs)
        out.append(prof)
    return out, units


def expected_profile(rna: bytes, records, p, seg_first=0, seg_count=-1):
    """The whole-set profile: the element-wise maximum of the records' profiles."""
    per, units = expected_profiles(rna, records, p, seg_first, seg_count)
    return np.maximum.reduce(per), units


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _tie_to_ssw_align(orc, rna, targets, what):
    """Fact 2 of section 13 on the units of one segment: where the reference's column maxima all stay below 148 its ssw_align
    returns sw_score == max_i R_unit[i] and R_unit[query_end] == sw_score.  Returns (units compared, units left out)."""
    cm, rm = rowmax_units(rna, targets)
    compared = left_out = 0
    for k, t in enumerate(targets):
        if max(orc.pre_align(rna, t)) >= 148:
            left_out += 1
            continue
        (sw_score, _, _, _, query_end), _ = orc.align(rna, t)
        assert sw_score == int(rm[k].max()), (what, k, sw_score, int(rm[k].max()))
        assert int(rm[k][query_end]) == sw_score, (what, k, query_end, int(rm[k][query_end]), sw_score)
        assert int(cm[k].max()) == sw_score, (what, k)
        compared += 1
    return compared, left_out


def test_restatement_rows_and_columns(oracle_build, golden_dir):
    """The column maxima of rowmax_units are those of colmax_units (the yardstick of the potential tracks), max_i R == max_x P
    for every demo unit, and a scalar double loop gives the same rows and columns on 600 columns of the hottest unit."""
    rna = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    dna = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    targets = [encode_unit(dna, e) for e in range(48)]
    cm, rm = rowmax_units(rna, targets)
    assert rm.shape == (48, len(rna))
    assert np.array_equal(cm, colmax_units(rna, targets))
    assert cm.max(axis=1).tolist() == rm.max(axis=1).tolist()          # fact 1, unit by unit
    hot = int(np.argmax(cm.max(axis=1)))
    assert int(cm[hot].max()) > 250
    cm6, rm6 = rowmax_units(rna, [targets[hot][:600]])
    cols, rows = rowmax_scalar(rna, targets[hot][:600])
    assert cm6[0].tolist() == cols and rm6[0].tolist() == rows


def test_restatement_equals_ssw_align_below_148(oracle_build, golden_dir):
    """The oracle tie on the 48 demo units and on the 48 units of each of the first six MEG3 peaks (cut to 5 000 nt: one segment).
    Units whose reference column maxima reach 148 are left out, at most 5 % of them (the reference alone leaves out 0 % and
    0.35 %)."""
    orc = helpers.Oracle(oracle_build)
    h19 = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    assert len(demo) <= 5000
    compared, left_out = _tie_to_ssw_align(orc, h19, [orc.encode_unit(demo, e)[0] for e in range(48)], "demo")
    print(f"demo: {compared} units compared, {left_out} left out")
    assert compared + left_out == 48 and compared >= 20
    meg3 = synth.read_fasta(os.path.join(golden_dir, "MEG3.fa"))[1]
    compared = left_out = 0
    for k, (_, dna) in enumerate(helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:6]):
        c, o = _tie_to_ssw_align(orc, meg3, [orc.encode_unit(dna[:5000], e)[0] for e in range(48)], f"peak {k}")
        compared, left_out = compared + c, left_out + o
    print(f"MEG3 peaks: {compared} units compared, {left_out} left out")
    assert compared + left_out == 6 * 48
    assert left_out <= 0.05 * (compared + left_out)


def test_profile_merge_is_the_maximum(mod):
    rng = np.random.default_rng(7)
    parts = [rng.integers(0, 16384, size=(4, 131)).astype(np.uint16) for _ in range(3)]
    profs = [mod.TfoProfile(a, units=k + 1, saturated_units=k) for k, a in enumerate(parts)]
    got = mod.merge_tfo_profiles(profs)
    assert (got.m, got.units, got.saturated_units) == (131, 6, 3)
    arr = got.array()
    assert arr.dtype == np.uint16 and arr.shape == (4, 131)
    assert np.array_equal(arr, np.maximum(np.maximum(parts[0], parts[1]), parts[2]))
    assert np.array_equal(mod.merge_tfo_profiles(profs[:1]).array(), parts[0])
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_tfo_profiles([profs[0], mod.TfoProfile(parts[1][:, :130])])
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_tfo_profiles([])
    assert ei.value.code == mod.E_ARG


def test_profile_tsv_bytes(mod):
    """Header, then one tab-separated line per base: 1-based position, the letter as given, the four classes in order."""
    v = np.zeros((4, 5), dtype=np.uint16)
    v[0] = [0, 5, 10, 15, 11]
    v[1, 4] = 16383
    v[3, 0] = 7
    want = HEADER + b"1\tA\t0\t0\t0\t7\n2\tc\t5\t0\t0\t0\n3\tU\t10\t0\t0\t0\n4\tn\t15\t0\t0\t0\n5\tG\t11\t16383\t0\t0\n"
    assert mod.tfo_profile_tsv(mod.TfoProfile(v), b"AcUnG", "toy") == want
    with pytest.raises(mod.FasimError) as ei:
        mod.tfo_profile_tsv(mod.TfoProfile(v), b"ACGT", "toy")
    assert ei.value.code == mod.E_ARG


def test_profile_symbols_are_exported(mod):
    for s in ("fasim_scan_tfo_profile", "fasim_tfo_profile_merge", "fasim_tfo_profile_tsv", "fasim_tfo_profile_free"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    for s in ("TfoProfile", "merge_tfo_profiles", "tfo_profile_tsv"):
        assert hasattr(mod, s)
    assert hasattr(mod.Engine, "scan_tfo_profile")
