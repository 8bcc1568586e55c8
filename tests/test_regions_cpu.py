"""BED intervals for region scans (fasim_read_bed, read_bed(), `fasim --regions`): the parser's rules and refusals, and the CLI's
usage errors.  None of these cases reaches a device: every refusal happens before an engine is created."""
import os
import subprocess

import pytest

import __graft_entry__ as entry


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _bed(tmp_path, text, name="r.bed"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def _read(tmp_path, text):
    return [tuple(r) for r in _mod().read_bed(_bed(tmp_path, text))]


def test_comments_track_browser_and_blank_lines_are_skipped(tmp_path):
    text = ("# a comment\n"
            "track name=peaks description=\"MACS2\"\n"
            "browser position chr1:1-1000\n"
            "\n"
            "   \t \n"
            "chr1\t10\t20\n")
    assert _read(tmp_path, text) == [(6, "chr1", 10, 20, "chr1_11_20")]


def test_bed3_to_bed6_and_wider(tmp_path):
    text = ("chr1 0 5\n"                                           # BED3: name from the coordinates
            "chr1\t100\t200\tpeakA\n"                              # BED4
            "chr2\t7\t9\tpeakB\t500\t-\n"                          # BED6: score and strand ignored
            "chrX\t1\t3\tpeakC\t0\t+\t1\t3\t0\t1\t2,\t0,\n"        # BED12: everything after the name ignored
            "chr2 30 40\r\n")                                      # CRLF line end
    assert _read(tmp_path, text) == [
        (1, "chr1", 0, 5, "chr1_1_5"),
        (2, "chr1", 100, 200, "peakA"),
        (3, "chr2", 7, 9, "peakB"),
        (4, "chrX", 1, 3, "peakC"),
        (5, "chr2", 30, 40, "chr2_31_40"),
    ]


def test_duplicate_stems_get_the_line_appended(tmp_path):
    text = ("chr1\t0\t10\tp\n"
            "chr2\t0\t10\tp\n"          # same name, other chrom: another stem, kept
            "chr1\t5\t15\tp\n"          # same (name, chrom) as line 1
            "chr1\t0\t10\tp\n"          # identical to line 1
            "chr1\t1\t2\tp_3\n"         # collides with the renamed line 3
            "chr1\t0\t10\n"             # generated name
            "chr1\t0\t10\n")            # the same generated name
    names = [r[4] for r in _read(tmp_path, text)]
    assert names == ["p", "p", "p_3", "p_4", "p_3_5", "chr1_1_10", "chr1_1_10_7"]
    assert len({(r[1], r[4]) for r in _read(tmp_path, text)}) == 7


def test_empty_file_has_no_intervals(tmp_path):
    assert _read(tmp_path, "") == []
    assert _read(tmp_path, "# only a comment\ntrack name=x\n") == []


BAD = [
    ("chr1\t10\n", 1, "fewer than 3 columns"),
    ("# header\nchr1\t1\t5\nchr1 5\n", 3, "fewer than 3 columns"),
    ("chr1\t1.5\t20\n", 1, "not an integer"),
    ("chr1\t1\t2e3\n", 1, "not an integer"),
    ("chr1\tten\t20\n", 1, "not an integer"),
    ("chr1\t1\t99999999999999999999999\n", 1, "not an integer"),
    ("chr1\t5\t9\nchr1\t-1\t20\n", 2, "start -1 < 0"),
    ("chr1\t20\t20\n", 1, "end 20 <= start 20"),
    ("chr1\t0\t10\nchr1\t20\t10\n", 2, "end 10 <= start 20"),
    ("chr1\t0\t2147483648\n", 1, "longer than 2^31 - 1"),
]


@pytest.mark.parametrize("text,line,reason", BAD, ids=[b[2].split()[0] + str(i) for i, b in enumerate(BAD)])
def test_refusals_name_the_line_and_the_reason(tmp_path, text, line, reason):
    m = _mod()
    with pytest.raises(m.FasimError) as ei:
        m.read_bed(_bed(tmp_path, text))
    assert ei.value.code == m.E_ARG
    assert f"line {line}:" in str(ei.value) and reason in str(ei.value), str(ei.value)


def test_longest_interval_is_accepted(tmp_path):
    assert _read(tmp_path, "chr1\t1\t2147483648\n") == [(1, "chr1", 1, 2147483648, "chr1_2_2147483648")]


def test_missing_file_is_refused(tmp_path):
    m = _mod()
    with pytest.raises(m.FasimError) as ei:
        m.read_bed(str(tmp_path / "missing.bed"))
    assert ei.value.code == m.E_ARG and "cannot read" in str(ei.value)


# ---- the CLI: usage errors and bad files exit 2 before any engine exists and write nothing --------------------------------------
def _cli(tmp_path, *args):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    return r, sorted(os.listdir(out))


@pytest.mark.parametrize("text,line,reason", BAD, ids=[b[2].split()[0] + str(i) for i, b in enumerate(BAD)])
def test_cli_exits_2_on_a_bad_bed_file(tmp_path, text, line, reason):
    _bed(tmp_path, text)
    r, written = _cli(tmp_path, "--regions", "r.bed")
    assert r.returncode == 2, r.stderr
    assert f"line {line}:" in r.stderr and reason in r.stderr, r.stderr
    assert written == []


@pytest.mark.parametrize("other", ["--all-records", "--accumulate-records"])
def test_cli_regions_excludes_record_modes(tmp_path, other):
    _bed(tmp_path, "chr1\t0\t50\n")
    r, written = _cli(tmp_path, "--regions", "r.bed", other)
    assert r.returncode == 2 and "--regions excludes" in r.stderr, r.stderr
    assert written == []


def test_cli_missing_bed_file_exits_2(tmp_path):
    r, written = _cli(tmp_path, "--regions", "missing.bed")
    assert r.returncode == 2 and "cannot read BED file" in r.stderr and "missing.bed" in r.stderr, r.stderr
    assert written == []


def test_cli_empty_bed_writes_only_the_index_header(tmp_path):
    _bed(tmp_path, "# nothing to scan\n")
    r, written = _cli(tmp_path, "--regions", "r.bed")
    assert r.returncode == 0, r.stderr
    assert written == ["Q-g.regions.tsv"]
    assert (tmp_path / "out" / "Q-g.regions.tsv").read_text() == "line\tname\tchrom\tstart\tend\tsegments\ttriplexes\tstem\n"
