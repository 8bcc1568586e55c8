"""csrc/call_plan.h -- the segment table of a call and its cuts into batches -- through the stand-alone driver tests/call_plan_main.cpp,
against a restatement of the rules in Python (written from the rules below, not from the header):

  * a record of n bases is cut at step = cutLength - overlapLength: one segment per start in range(0, n, step), cutLength long or to
    the record's end;
  * the segments of a record set are numbered globally, record after record; a call selects [seg_first, seg_first + seg_count) of
    that list, seg_first below 0 meaning 0 and a seg_count below 0 or past the end meaning "to the end";
  * cut by bases: a batch closes as soon as it holds `cap` segments or at least `target` bases, what is left is the last batch;
  * fixed cut: batches of seg_batch segments, batches that start in the last taper_pct percent of the segments half that (at least 1).

Two anchors come from the project's record, not from the code under test: the batch shape in the comment of scan_set (engine_scan.cpp)
and the cases of test_host_cpu.test_segment_count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# driver commands (tests/call_plan_main.cpp); records are LEN or OFF:LEN
CASES = [
    ("table", 5000, 100, 0, -1, 4899),                              # one record shorter than a segment ...
    ("table", 5000, 100, 0, -1, 1),
    ("table", 5000, 100, 0, -1, 3 * 4900),                          # ... of exactly k * step, and one base more
    ("table", 5000, 100, 0, -1, 3 * 4900 + 1),
    ("table", 5000, 100, 0, -1, 1, 4999, 5001),                     # three records around one segment
    ("table", 5000, 100, 0, -1, "70:1", "10:4999", "90000:5001"),   # ... anywhere in the buffer, overlapping
    ("table", 5000, 100, 2, -1, 1, 4999, 5001),                     # seg_first inside the second record
    ("table", 5000, 100, 2, 100, 1, 4999, 5001),                    # seg_count past the end
    ("table", 5000, 100, 9, 4, 1, 4999, 5001),                      # seg_first past the end
    ("table", 5000, 100, -7, 2, 1, 4999, 5001),                     # seg_first below 0
    ("table", 5000, 100, 1, 0, 1, 4999, 5001),                      # seg_count = 0
    ("table", 5000, 100, 1, 2, 1, 4999, 5001),                      # a range that ends on a record boundary
    ("table", 5000, 100, 0, 3, 1, 4999, 5001),
    ("table", 64, 13, 3, 11, 51, 52, 1, 200, 102),                  # another cut: step 51
    ("table", 7, 0, 0, -1, 7, 8, 6, 14),                            # no overlap
    ("bases", 5000, 100, 0, -1, 1, 1 << 40, 1, 4999, 5001),         # cap = 1: every segment its own batch
    ("bases", 5000, 100, 0, -1, 1000, 50, 1, 4999, 5001),           # a target smaller than one segment: the 1-base segment alone too
    ("bases", 5000, 100, 0, -1, 1000, 5100, 1, 4999, 5001, 9800),   # batches that cross records, the last one left open
    ("bases", 5000, 100, 0, -1, 1000, 5000, 5000, 5000),            # ... and one that closes on the last segment: nothing left
    ("bases", 5000, 100, 0, -1, 2, 1 << 40, 30000),                 # cap alone closes; 7 segments: the last batch holds one
    ("bases", 5000, 100, 3, 4, 3, 9000, 1, 4999, 5001, 30000),      # a range of the list, cut from its own first segment
    ("bases", 5000, 100, 1, 0, 3, 9000, 1, 4999, 5001),             # nothing selected: no batch
    ("fixed", 10, 3, 0),
    ("fixed", 9, 3, 0),
    ("fixed", 1000, 384, 0),
    ("fixed", 0, 384, 25),
    ("fixed", 10, 1, 25),                                           # half of 1 is still 1
    ("fixed", 100, 8, 25),
    ("fixed", 101, 7, 25),                                          # a full batch that starts before the taper and ends inside it
    ("fixed", 10204, 511, 25),
]


def _records(specs):
    out, nxt = [], 0
    for s in specs:
        off, n = (int(x) for x in s.split(":")) if isinstance(s, str) else (nxt, s)
        out.append((off, n))
        nxt = off + n
    return out


def _table(cut, overlap, seg_first, seg_count, specs):
    step = cut - overlap
    recs = _records(specs)
    segs, first = [], [0]
    for r, (off, n) in enumerate(recs):
        segs += [(r, i, off + pos, min(cut, n - pos)) for i, pos in enumerate(range(0, n, step))]
        first.append(len(segs))
    seg_first = max(0, seg_first)
    rows = segs[seg_first:] if seg_count < 0 else segs[seg_first:seg_first + seg_count]
    return seg_first, rows, first


def expected(case):
    """The driver's output for `case`, from the rules in this module's docstring."""
    kind, a = case[0], case[1:]
    if kind == "table":
        seg_first, rows, first = _table(a[0], a[1], a[2], a[3], a[4:])
        return ([f"range {seg_first} {len(rows)} {sum(x[3] for x in rows)}", "first " + " ".join(str(x) for x in first)] +
                [f"seg {r} {i} {off} {n}" for r, i, off, n in rows])
    if kind == "bases":
        _, rows, _ = _table(a[0], a[1], a[2], a[3], a[6:])
        cap, target = a[4], a[5]
        out, b0, bases = [], 0, 0
        for s, row in enumerate(rows):
            bases += row[3]
            if s + 1 - b0 == cap or bases >= target:
                out.append(f"chunk {b0} {s + 1}")
                b0, bases = s + 1, 0
        return out + ([f"chunk {b0} {len(rows)}"] if b0 < len(rows) else [])
    n, batch, taper = a
    tail = n * taper // 100          # the segments of the taper
    out, b0 = [], 0
    while b0 < n:
        size = max(1, batch // 2) if taper > 0 and b0 >= n - tail else batch
        out.append(f"chunk {b0} {min(n, b0 + size)}")
        b0 = min(n, b0 + size)
    return out


def _line(case):
    return " ".join(str(x) for x in case)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/call_plan_main.cpp built with the host C++ compiler: call_plan.h needs neither HIP nor the engine."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("call_plan") / "call_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "call_plan_main.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def printed(driver, tmp_path_factory):
    """One run of the driver over all CASES: {command line: its output lines}."""
    path = tmp_path_factory.mktemp("call_plan_cases") / "cases.txt"
    path.write_text("".join(_line(c) + "\n" for c in CASES))
    text = subprocess.run([driver, "@" + str(path)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith("# "):
            cur = out.setdefault(ln[2:], [])
        else:
            cur.append(ln)
    return out


@pytest.mark.parametrize("case", CASES, ids=_line)
def test_plan_matches_the_rules(printed, case):
    assert printed[_line(case)] == expected(case)


def test_batch_shape_of_the_50mb_record(printed):
    """The comment in scan_set: 50 Mb = 10 204 segments on ten workers -> seg_batch 511, taper 25: 15 batches of 511, then 10 of
    at most 255 (by hand: 7 665 segments in full batches, the tapered 2 539 = 9 x 255 + 244)."""
    sizes = [int(b) - int(a) for _, a, b in (ln.split() for ln in printed["fixed 10204 511 25"])]
    assert sizes == [511] * 15 + [255] * 9 + [244]


def test_segment_count_matches_the_library(driver):
    """segment_count of call_plan.h == fasim_segment_count on the cases of test_host_cpu.test_segment_count."""
    import __graft_entry__ as entry
    m = entry.load()
    ns = (1, 4899, 4900, 4901, 5000, 9800, 9801, 50_000_000)
    text = subprocess.run([driver, "count", "5000", "100"] + [str(n) for n in ns], check=True, capture_output=True, text=True).stdout
    got = [int(ln.split()[1]) for ln in text.splitlines()]
    assert got == [m.segment_count(n) for n in ns] == [len(range(0, n, 4900)) for n in ns]
