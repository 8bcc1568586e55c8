"""The hits of oligo sites (fasim_scan_oligos_aligned), the part that needs no GPU: the fact that
k_site_ends_short is built on -- the end cell and the start cell of a site's hit are decided by a window of the unit, not by its
prefix -- as a numpy restatement of the kernel's passes (i) and (ii) (zero state at (jp & ~15) - warm, code N before column 0 and
behind the unit, the echo window of npad columns, at most W(m) reverse columns) against the yardstick of section 15
(test_site_align_cpu.py::unit_matrix + align_in_unit, over the whole prefix); the exported symbols, the option key and the table of
a hand-made oligo hit list; the refusals of `fasim --oligo-hits`."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import _CODE, encode_unit
from test_oligos_cpu import OLIGOS_OK, warmup
from test_site_align_cpu import _anchored, _hand_made, _row, align_in_unit, unit_matrix


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


# ---- 1. the window is exact --------------------------------------------------------------------------------------------------------
def warm_columns(m: int) -> int:
    """Columns before (jp & ~15) at which pass (i) starts from zeros: W(m) + 16, rounded up to 16."""
    return (warmup(m) + 16 + 15) // 16 * 16


def window_ends(rna: bytes, target: bytes, jp: int, value: int):
    """Passes (i) and (ii) as k_site_ends_short does them: (i1, j1, i0, j0), i1 == -1: the unit does not attain `value` in column
    jp; i0 == -1: the reverse pass did not reach `value` within W(m) columns."""
    m, n = len(rna), len(target)
    rows = 16 * ((m + 15) // 16)
    npad = rows - m
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = np.full((n + 15) // 16 * 16, 4, dtype=np.int64)              # the host pads a unit's row to a multiple of 16 with code N
    t[:n] = _CODE[np.frombuffer(target, dtype=np.uint8)]
    prof = np.full((5, rows), -4, dtype=np.int64)                    # pad rows score -4 here: they are computed and never looked at
    for c in range(4):
        prof[c, :m] = np.where(q == c, 5, -4)
    ramp = 4 * np.arange(rows, dtype=np.int64)
    h = np.zeros(rows, dtype=np.int64)
    e = np.zeros(rows, dtype=np.int64)
    c_lo = max(0, jp - npad)
    i1 = j1 = -1
    att = False
    for c in range((jp & ~15) - warm_columns(m), (jp | 15) + 1):
        code = t[c] if c >= 0 else 4
        diag = np.zeros(rows, dtype=np.int64)
        diag[1:] = h[:-1]
        e = np.maximum(e - 4, h - 16)
        hp = np.maximum(np.maximum(diag + prof[code], e), 0)
        run = np.maximum.accumulate(hp + ramp)
        f = np.zeros(rows, dtype=np.int64)
        f[1:] = run[:-1] - ramp[1:] - 12
        h = np.maximum(hp, f)
        if c_lo <= c <= jp:
            hit = np.flatnonzero(h[:m] == value)
            if len(hit):
                j1, i1 = c, int(hit[0])
                att = att or c == jp or int(h[m - 1]) == value
    if not att:
        return -1, -1, -1, -1
    cols = min(j1 + 1, warmup(m))
    s = prof[t[j1 + 1 - cols:j1 + 1]][:, :i1 + 1].T[::-1, ::-1]     # rows i1 .. 0, columns j1 .. j1 - cols + 1
    dd = _anchored(s)[3]
    found = np.flatnonzero((dd == value).any(axis=0))
    if not len(found):
        return i1, j1, -1, -1
    c = int(found[0])
    return i1, j1, i1 - int(np.flatnonzero(dd[:, c] == value)[0]), j1 - c


def _gt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"GT", dtype=np.uint8), size=n).tobytes())


def _for_enc(piece: bytes, enc: int) -> bytes:
    """DNA whose unit under `enc` reads `piece` (letters the rule puts out)."""
    inv = {}
    for base, o in zip("ATGC", synth.RULE_OUT[enc]):
        inv.setdefault(o, base)
    d = "".join(inv[chr(c)] for c in piece).encode()
    return d[::-1] if enc & 1 else d


def _unit_with_plants(rng, oligo: bytes, first_end: int):
    """The letters of a unit: the oligo ending in column first_end, then copies of it with a DNA-side insertion of every length
    up to (5 m - 13) div 4 in the middle, one with two query bases missing, one with a mismatch, one whole copy in the unit's
    last columns; between them short random stretches.  Returns the letters and the last column of every plant."""
    m = len(oligo)
    dmax = max(0, (5 * m - 13) // 4)
    h = m // 2
    flip = bytes([oligo[h] ^ (ord("G") ^ ord("T"))])
    plants = [oligo[:h] + _gt(rng, d) + oligo[h:] for d in range(1, dmax + 1)]
    plants += [oligo[:h] + oligo[h + 2:], oligo[:h] + flip + oligo[h + 1:]]
    t = bytearray(_gt(rng, first_end + 1 - m) + oligo)
    ends = [len(t) - 1]
    for x in plants:
        t += _gt(rng, int(rng.integers(1, 9))) + x
        ends.append(len(t) - 1)
    t += _gt(rng, warm_columns(m) + 40) + oligo
    ends.append(len(t) - 1)
    return bytes(t), ends


@pytest.mark.parametrize("enc", [0, 1])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 20, 33, 112])
def test_the_window_gives_the_end_and_start_cell_of_the_prefix(m, enc):
    """Every problem (a column jp whose maximum is the value) of a planted unit: the windowed passes give the (i0, i1, j0, j1) of
    unit_matrix + align_in_unit.  Peaks at columns 0, 1, warm - 1 (first unit) or warm (second unit) and n - 1, at the end of every
    plant and up to npad columns behind some (there the column's maximum is a pad row's echo), and a dozen columns anywhere; and,
    with a value one above the column's maximum, a problem whose unit does not attain the value.  A column whose maximum is below
    that of the column before it is no problem of a site (its maximum may be the end of a gap, which no peak of a potential is)
    and is left out."""
    rng = np.random.default_rng(1800 + 2 * m + enc)
    oligo = _gt(rng, m)
    npad = 16 * ((m + 15) // 16) - m
    warm = warm_columns(m)
    echoes = gapped = 0
    for k in (0, 1):
        letters, ends = _unit_with_plants(rng, oligo, warm - 1 + k)
        seg = _for_enc(letters, enc)
        target = encode_unit(seg, enc)
        assert target == letters                              # (forward: the rule's letters; mirrored: the segment read backwards)
        n = len(target)
        H = unit_matrix(oligo, target)
        cm = H.max(axis=0)
        assert n > 2 * warm and int(cm.max()) == 5 * m and ends[0] == warm - 1 + k and ends[-1] == n - 1
        must = {0, 1, warm - 1 + k, n - 1}
        cols = must | set(ends)
        for d in (1, npad // 2, npad):
            cols |= {min(n - 1, x + d) for x in ends[::7]}
        cols |= {int(x) for x in rng.integers(0, n, size=12)}
        for jp in sorted(cols):
            value = int(cm[jp])
            if value < 1 or (jp > 0 and cm[jp] < cm[jp - 1]):
                assert jp not in must or (m == 1 and value < 1), (m, enc, k, jp)
                continue
            want = align_in_unit(oligo, target, H, jp, value)
            got = window_ends(oligo, target, jp, value)
            assert got == (want[1], want[3], want[0], want[2]), (m, enc, k, jp, value, got, want)
            echoes += int(H[:m, jp].max()) < value
            gapped += "D" in want[4]
            assert window_ends(oligo, target, jp, value + 1)[0] == -1, (m, enc, k, jp)
    if npad:
        assert echoes >= 1, "no column whose maximum is only a pad row's echo"
    if m >= 15:
        assert gapped >= 1


def test_a_gapped_plant_at_the_end_of_the_unit():
    """One plant whose gapped alignment beats either half, ending on the unit's last column: the hit spans m + d <= W(m) columns
    and the window finds both of its cells."""
    m = 20
    rng = np.random.default_rng(1820)
    oligo = _gt(rng, m)
    d = 5                                                     # 5 * 10 > 4 * 5 + 12: the gapped alignment beats either half
    target = _gt(rng, 300) + oligo[:10] + b"A" * d + oligo[10:]
    H = unit_matrix(oligo, target)
    jp = len(target) - 1
    value = int(H[:, jp].max())
    assert value == 5 * m - 4 * d - 12
    want = align_in_unit(oligo, target, H, jp, value)
    assert window_ends(oligo, target, jp, value) == (want[1], want[3], want[0], want[2]) and want[3] - want[2] + 1 == m + d
    assert want[3] - want[2] + 1 <= warmup(m)


# ---- 2. exports and tables ---------------------------------------------------------------------------------------------------------
def test_symbols_and_the_option_key(mod):
    assert "fasim_scan_oligos_aligned" in mod.EXPORTS and hasattr(mod.lib(), "fasim_scan_oligos_aligned")
    assert hasattr(mod.Engine, "scan_oligos_aligned")
    src = open(os.path.join(entry.PKG_DIR, "csrc", "engine.cpp")).read()
    assert '"site_short"' in src                              # (fasim_set_option needs an engine, an engine a GPU: test_gpu_oligo_hits.py sets it)


def test_table_of_a_hand_made_oligo_hit_list(mod):
    make, keep = _hand_made(mod)
    sites = mod.Sites([(0, 100, 112, 41, 109, 0), (3, 300, 305, 30, 302, 13), (2, 400, 401, 37, 400, 12)], min_value=30, max_gap=1)
    h = make([_row(0, 0, [(10 << 4)]),
              _row(1, 13, [(4 << 4), (2 << 4) | 2, (5 << 4)], stari=1, endi=9, starj=295, endj=305, nt=11, identity=81.8182, tri=0.75,
                   tfo="GGAG--GGAGA", tts="GGAGTTGGAGA"),
              _row(-1, 12, None)])
    got = mod.site_hits_tsv(sites, h, "chr2", 501, "tfo20", record_name="peak_7")
    want = (b"# fasim site hits lncRNA=tfo20 min_value=30 max_gap=1\n"
            b"chrom\ttts_start\ttts_end\tclass\tvalue\tstrand\trule\ttfo_start\ttfo_end\tnt\tidentity\tstability\tcigar\tTFO\tTTS\tname\n"
            b"chr2\t600\t610\tParaPlus\t41\t+\t1\t3\t12\t10\t90\t1.25\t10M\tACGUACGUAC\tACGTACGTAC\tpeak_7\n"
            b"chr2\t795\t806\tAntiPlus\t30\t+\t1\t1\t9\t11\t81.8182\t0.75\t4M2D5M\tGGAG--GGAGA\tGGAGTTGGAGA\tpeak_7\n"
            b"chr2\t900\t901\tAntiMinus\t37\t-\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tpeak_7\n")
    assert got == want
    del h


# ---- 3. the CLI's refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--sites", "60", "--oligo-hits"], ["--oligos", "--oligo-hits"],
                                  ["--oligos", "--potential-hist", "--oligo-hits"], ["--oligos", "--sites", "60", "--sites-align"],
                                  ["--oligos", "--sites", "60", "--sites-align", "--oligo-hits"]])
def test_cli_refusals_write_nothing(tmp_path, args):
    """--oligo-hits without --oligos, without --sites, with --potential-hist; --oligos --sites V --sites-align stays refused."""
    exe = os.path.join(entry.PKG_DIR, "fasim")
    gold = os.path.join(entry.ROOT, "tests", "golden")
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    (tmp_path / "in" / "oligos.fa").write_bytes(OLIGOS_OK)
    r = subprocess.run([exe, "-f1", os.path.join(gold, "testDNA.fa"), "-f2", str(tmp_path / "in" / "oligos.fa"), "-O", str(tmp_path / "out") + "/"] + args,
                       capture_output=True)
    assert r.returncode == 2, r.stderr
    assert os.listdir(tmp_path / "out") == []
