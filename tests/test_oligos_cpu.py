"""Panels of short oligos (fasim_scan_oligos), the part that needs no GPU: the exported symbols, the panel
table fasim_oligo_panel_tsv, the refusals of `fasim --oligos`, and the fact k_scan_short is built on -- the alignments that decide a
column maximum start at most W(m) columns before it, so a DP started from zeros W(m) columns early is exact from there on --
checked against the restatement of the definition (test_track_cpu.py::colmax_units)."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_track_cpu import colmax_units


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def warmup(m: int) -> int:
    """W(m) of DESIGN.md section 16: at most 16 * ceil(m / 16) pairs, and DNA-side gap residues of cost 4 D + 12 < 5 m."""
    return 16 * ((m + 15) // 16) + max(0, (5 * m - 13) // 4)


def test_symbols_and_constants_are_exported(mod):
    for s in ("fasim_scan_oligos", "fasim_oligo_panel_tsv"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    assert mod.MAX_OLIGO == 112
    assert hasattr(mod.Engine, "scan_oligos") and callable(mod.oligo_panel_tsv)
    assert [warmup(m) for m in (1, 20, 112)] == [16, 53, 248]


def test_panel_table_bytes(mod):
    """Sums and maxima over all records; a class without a site has 0 in its maximum, an oligo without any site a line of zeros."""
    a0 = mod.Sites([[0, 5, 10, 60, 7, 0], [3, 20, 24, 80, 21, 13], [0, 30, 31, 75, 30, 0]], min_value=60)
    a1 = mod.Sites([[0, 100, 140, 66, 120, 1], [2, 0, 3, 61, 1, 12]], min_value=60)
    none = mod.Sites([], min_value=60)
    got = mod.oligo_panel_tsv(["tfo_a", "tfo_b", "tfo_c"], [b"ACGTACGTACGTACGTACGT", b"GA", b"T" * 112], [[a0, a1], [none, none], [none, a1]])
    head = "oligo\tlength\ttotal_sites\tcovered_bases"
    for c in ("ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus"):
        head += f"\t{c}_sites\t{c}_max"
    want = (head + "\n"
            "tfo_a\t20\t5\t53\t3\t75\t0\t0\t1\t61\t1\t80\n"
            "tfo_b\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n"
            "tfo_c\t112\t2\t43\t1\t66\t0\t0\t1\t61\t0\t0\n")
    assert got == want.encode()
    assert mod.oligo_panel_tsv([], [], []) == (head + "\n").encode()
    for bad in ((["a"], [b"AC"], []), (["a", "b"], [b"AC", b"AC"], [[none, none], [none]])):
        with pytest.raises(mod.FasimError) as ei:
            mod.oligo_panel_tsv(*bad)
        assert ei.value.code == mod.E_ARG


OLIGOS_OK = b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>tfo2\nTTCTTCTCCTTTCTCTTTCC\n"
CLI_REFUSALS = [
    (OLIGOS_OK, ["--oligos"]),
    (OLIGOS_OK, ["--oligos", "--sites-gap", "3"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--sites-align"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "-F"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--track", "25"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--all-records", "--screen"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--tfo-profile"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--accumulate-records"]),
    (OLIGOS_OK, ["--oligos", "--sites", "0"]),
    (b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>hollow\n>tfo3\nGGA\n", ["--oligos", "--sites", "60"]),
    (b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>long113\n" + b"GA" * 56 + b"G\n", ["--oligos", "--sites", "60"]),
]


@pytest.mark.parametrize("case", range(len(CLI_REFUSALS)))
def test_cli_refusals_write_nothing(tmp_path, case):
    """Status 2 before any device is opened, nothing written; an -f2 record that is no oligo is named."""
    panel, args = CLI_REFUSALS[case]
    exe = os.path.join(entry.PKG_DIR, "fasim")
    gold = os.path.join(entry.ROOT, "tests", "golden")
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    (tmp_path / "in" / "oligos.fa").write_bytes(panel)
    r = subprocess.run([exe, "-f1", os.path.join(gold, "testDNA.fa"), "-f2", str(tmp_path / "in" / "oligos.fa"), "-O", str(tmp_path / "out") + "/"] + args,
                       capture_output=True)
    assert r.returncode == 2, r.stderr
    assert os.listdir(tmp_path / "out") == []
    for name in (b"hollow", b"long113"):
        if name in panel:
            assert name in r.stderr and b"112" in r.stderr


def _plant(rng, oligo: bytes, gap: int) -> bytes:
    """half, a DNA-side insertion of `gap` random bases, half"""
    h = len(oligo) // 2
    return oligo[:h] + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=gap).tobytes()) + oligo[h:]


@pytest.mark.parametrize("m", [1, 16, 17, 20, 112])
def test_a_dp_started_w_columns_early_is_exact(m):
    """Targets that carry the oligo itself with DNA-side insertions of every affordable length (up to (5 m - 13) div 4 residues, where the
    two halves still pay for the gap) and chains of such plants: the column maxima of the target cut at several offsets equal those of
    the whole target from offset + W(m) on.  One column earlier they need not: the bound is not checked for slack, only for safety."""
    rng = np.random.default_rng(1600 + m)
    oligo = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=m).tobytes())
    w = warmup(m)
    dmax = max(0, (5 * m - 13) // 4)
    gaps = sorted({0, 1, dmax // 2, max(0, dmax - 1), dmax})
    target = bytearray(synth.random_dna(200, 16 + m))
    for g in gaps + gaps:
        target += _plant(rng, oligo, g) + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(0, 9))).tobytes())
    target += synth.random_dna(w + 40, 17 + m)
    target = bytes(target)
    full = colmax_units(oligo, [target])[0]
    assert int(full.max()) >= min(5 * m, 5 * (m // 2) + 1)
    offsets = sorted({1, 97, 200 + m // 2, 200 + m + dmax // 2, len(target) // 2, len(target) - w - 20})
    for off in offsets:
        cut = colmax_units(oligo, [target[off:]])[0]
        assert np.array_equal(cut[w:], full[off + w:]), (m, off)
