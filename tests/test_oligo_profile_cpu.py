"""Per-base profiles and screens of oligo panels (fasim_scan_oligos_profile, fasim_scan_oligos_peaks), the part
that needs no GPU: the exported symbols; the yardstick of the GPU tests (test_tfo_profile_cpu.py::rowmax_units, which takes any m)
tied to the reference's own ssw_align for oligos of at most 29 nt, where nothing has to be left out; the fact that makes
k_scan_short_rows mask its columns -- one column of code N behind a unit raises a row above everything it really holds --; and the
refusals of `fasim --oligos --oligo-profile / --oligo-screen`."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import synth
import __graft_entry__ as entry
from test_tfo_profile_cpu import _tie_to_ssw_align, rowmax_scalar, rowmax_units


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def test_symbols_are_exported(mod):
    for s in ("fasim_scan_oligos_profile", "fasim_scan_oligos_peaks"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    for s in ("scan_oligos_profile", "scan_oligos_peaks"):
        assert hasattr(mod.Engine, s)
    for s in ("TfoProfile", "merge_tfo_profiles", "tfo_profile_tsv", "merge_peaks", "screen_tsv"):
        assert hasattr(mod, s)


@pytest.mark.parametrize("m", [1, 7, 16, 17, 112])
def test_restatement_takes_any_length(m):
    """rowmax_units against the scalar double loop for the lengths around the pad-row edge."""
    rng = np.random.default_rng(2400 + m)
    oligo = bytes(rng.choice(np.frombuffer(b"ACGU", dtype=np.uint8), size=m).tobytes())
    target = bytearray(synth.random_dna(300, 24 + m))
    target[120:120 + m] = oligo.replace(b"U", b"A")
    cm, rm = rowmax_units(oligo, [bytes(target)])
    cols, rows = rowmax_scalar(oligo, bytes(target))
    assert rm.shape == (1, m) and cm[0].tolist() == cols and rm[0].tolist() == rows
    assert int(rm[0][m - 1]) == 5 * m


def test_restatement_equals_ssw_align_for_oligos(oracle_build, golden_dir):
    """The oracle tie on the 48 demo units for oligos of 1 .. 29 nt cut from H19: 5 * 29 = 145 < 148, so no unit is left out."""
    orc = helpers.Oracle(oracle_build)
    h19 = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]
    demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))[1]
    targets = [orc.encode_unit(demo, e)[0] for e in range(48)]
    for k, m in enumerate((1, 2, 15, 16, 17, 20, 29)):
        oligo = h19[300 + 131 * k:300 + 131 * k + m]
        compared, left_out = _tie_to_ssw_align(orc, oligo, targets, f"{m} nt")
        assert (compared, left_out) == (48, 0), (m, compared, left_out)


@pytest.mark.parametrize("m", [20, 33, 112])
def test_a_column_of_n_behind_the_unit_raises_a_row(m):
    """A target that ends in the oligo's first k = 3 m / 5 letters: row k - 1 holds 5 k on the last column, and a column of code N
    appended there continues the diagonal into row k at 5 k - 4, above everything row k really holds.  With sixteen such columns (the
    padding of a unit's row up to its stride) several rows go wrong.  So the row maxima must leave out the columns from n on."""
    rng = np.random.default_rng(2420 + m)
    oligo = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=m).tobytes())
    k = 3 * m // 5
    target = synth.random_dna(400, 25 + m) + oligo[:k]
    _, plain = rowmax_units(oligo, [target])
    _, one = rowmax_units(oligo, [target + b"N"])
    _, sixteen = rowmax_units(oligo, [target + b"N" * 16])
    assert int(plain[0][k - 1]) == 5 * k
    assert int(one[0][k]) == 5 * k - 4 > int(plain[0][k])
    wrong = int((sixteen[0] != plain[0]).sum())
    print(f"m = {m}: row {k} goes from {int(plain[0][k])} to {int(one[0][k])} with one N column; {wrong} rows differ with sixteen")
    assert wrong >= 2 and (sixteen >= plain).all()


OLIGOS_OK = b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>tfo2\nTTCTTCTCCTTTCTCTTTCC\n"
LNC = b">lnc\n" + b"GGAGGGAGAGGGAAGGAGAG" * 10 + b"\n"
CLI_REFUSALS = [
    (LNC, ["--oligo-profile"]),
    (LNC, ["--oligo-screen", "--all-records"]),
    (LNC, ["--sites", "60", "--oligo-profile"]),
    (OLIGOS_OK, ["--oligos", "--oligo-screen"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--oligo-screen"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--potential-hist"]),
    (OLIGOS_OK, ["--oligos", "--oligo-screen", "--all-records", "--potential-hist"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--oligo-hits", "--oligo-profile"]),
    (OLIGOS_OK, ["--oligos", "--sites", "60", "--oligo-hits", "--oligo-screen", "--all-records"]),
    # every refusal --oligos has, with the new flags in the place of --sites V
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--sites-gap", "3"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "-F"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--track", "25"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--all-records", "--screen"]),
    (OLIGOS_OK, ["--oligos", "--oligo-screen", "--all-records", "--screen"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--tfo-profile"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--accumulate-records"]),
    (OLIGOS_OK, ["--oligos", "--oligo-profile", "--sites", "0"]),
    (b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>hollow\n>tfo3\nGGA\n", ["--oligos", "--oligo-profile"]),
    (b">tfo1\nGGAGGGAGAGGGAAGGAGAG\n>long113\n" + b"GA" * 56 + b"G\n", ["--oligos", "--oligo-screen", "--all-records"]),
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
