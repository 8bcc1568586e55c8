"""Screening record sets by potential (fasim_scan_records_track), the part that needs no GPU: the exported
symbols, the two pure host functions of the C-ABI (fasim_peaks_merge, fasim_screen_tsv) and the option combinations the CLI
refuses before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def test_screen_symbols_are_exported(mod):
    for s in ("fasim_scan_records_track", "fasim_peaks_merge", "fasim_screen_tsv"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    for name in ("scan_records_track", "scan_regions_track"):
        assert callable(getattr(mod.Engine, name))
    assert callable(mod.merge_peaks) and callable(mod.screen_tsv)


def test_peaks_merge_orders_by_value_then_pos_then_enc(mod):
    """Rows are (value, pos, enc).  The larger value wins whatever the positions; equal values: the lower position; equal
    positions too: the lower encoding; a (0, -1, -1) entry loses against every real peak and survives only against itself."""
    none = (0, -1, -1)
    a = np.array([(5, 10, 3), none, (7, 4, 20), (7, 4, 2), (9, 0, 0), none, (3, 50, 40), (6, 8, 8)], dtype=np.int64)
    b = np.array([(5, 9, 7), none, (7, 4, 13), (8, 100, 40), none, (1, 700, 47), (3, 50, 40), (6, 9, 1)], dtype=np.int64)
    c = np.array([(4, 0, 0), none, (7, 5, 0), (8, 100, 41), none, (1, 699, 47), (3, 49, 41), (6, 8, 9)], dtype=np.int64)
    want2 = [(5, 9, 7), none, (7, 4, 13), (8, 100, 40), (9, 0, 0), (1, 700, 47), (3, 50, 40), (6, 8, 8)]
    want3 = [(5, 9, 7), none, (7, 4, 13), (8, 100, 40), (9, 0, 0), (1, 699, 47), (3, 49, 41), (6, 8, 8)]
    assert [tuple(x) for x in mod.merge_peaks([a, b]).tolist()] == want2
    assert [tuple(x) for x in mod.merge_peaks([b, a]).tolist()] == want2
    for order in ((a, b, c), (c, b, a), (b, c, a)):
        assert [tuple(x) for x in mod.merge_peaks(order).tolist()] == want3
    assert np.array_equal(mod.merge_peaks([a]), a)
    # the shape of the parts is kept: (records, 4, 3)
    got = mod.merge_peaks([a.reshape(2, 4, 3), b.reshape(2, 4, 3)])
    assert got.shape == (2, 4, 3) and got.dtype == np.int64 and [tuple(x) for x in got.reshape(-1, 3).tolist()] == want2
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_peaks([])
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_peaks([a, b[:4]])
    assert ei.value.code == mod.E_ARG


def test_screen_tsv_bytes(mod):
    """Hand-written: genome position = interval start + pos, Rule = enc // 2 + 1 (parallel, enc < 12) or (enc - 12) // 2 + 1
    (antiparallel), a zero peak prints 0 NA NA, an interval that was not scanned NA in every column after `end`."""
    R = mod.Region
    regs = [R(2, "chr7", 1000, 5900, "peak_a"), R(5, "chrX", 0, 12, "chrX_1_12"), R(6, "chr7", 1000, 5900, "peak_a_6")]
    peaks = np.array([[(137, 0, 0), (88, 4899, 11), (0, -1, -1), (251, 2040, 47)],
                      [(0, -1, -1)] * 4,
                      [(5, 7, 2), (16383, 3, 1), (40, 11, 12), (41, 0, 13)]], dtype=np.int64)
    head = "line\tname\tchrom\tstart\tend\tsegments"
    for c in ("ParaPlus", "ParaMinus", "AntiMinus", "AntiPlus"):
        head += f"\t{c}\t{c}_pos\t{c}_rule"
    want = (head + "\n" +
            "2\tpeak_a\tchr7\t1000\t5900\t1\t137\t1000\t1\t88\t5899\t6\t0\tNA\tNA\t251\t3040\t18\n" +
            "5\tchrX_1_12\tchrX\t0\t12" + "\tNA" * 13 + "\n" +
            "6\tpeak_a_6\tchr7\t1000\t5900\t3\t5\t1007\t2\t16383\t1003\t1\t40\t1011\t1\t41\t1000\t1\n")
    assert mod.screen_tsv(regs, [1, -1, 3], peaks) == want.encode()
    # scanned, nothing found: zeros, not NA, in the value columns
    zero = mod.screen_tsv(regs[1:2], [1], peaks[1:2]).decode().splitlines()[1]
    assert zero == "5\tchrX_1_12\tchrX\t0\t12\t1" + "\t0\tNA\tNA" * 4
    assert mod.screen_tsv([], [], np.zeros((0, 4, 3), dtype=np.int64)) == (head + "\n").encode()
    with pytest.raises(mod.FasimError) as ei:
        mod.screen_tsv(regs, [1, 1, 1], peaks[:2])
    assert ei.value.code == mod.E_ARG


def test_cli_refuses_before_any_work(mod, golden_dir, tmp_path):
    """--screen alone, with --accumulate-records, with -F, with --track under --regions (refused exactly as without --screen), and
    --screen-only with --track: exit status 2 and an empty output directory.  None of them reaches a device."""
    exe = os.path.join(entry.PKG_DIR, "fasim")
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    (tmp_path / "r.bed").write_text("chr11\t2158500\t2159000\n")
    cases = (["--screen"], ["--screen-only"], ["--screen", "--accumulate-records"], ["--screen", "--all-records", "-F"],
             ["--screen", "--regions", "r.bed", "-F"], ["--screen", "--track", "25", "--regions", "r.bed"],
             ["--screen-only", "--track", "25", "--regions", "r.bed"], ["--screen-only", "--all-records", "--track", "25"],
             ["--track", "25", "--regions", "r.bed"])
    for k, extra in enumerate(cases):
        out = tmp_path / f"out{k}"
        out.mkdir()
        r = subprocess.run([exe, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", f"out{k}/", *extra], cwd=tmp_path,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, (extra, r.returncode, r.stderr.decode())
        assert os.listdir(out) == [], extra
