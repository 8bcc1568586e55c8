"""csrc/doomed.h -- which alignments are certain to fail the stability filter, from their ends alone -- through the stand-alone driver
tests/doomed_main.cpp, against the scan's own record conversion (convert_triplex_num, host_post.cpp).

The driver draws random alignments: spans 1-120, CIGARs with I and D runs, both strands, reversed encodings, segments with N and IUPAC
letters, and planted ones: the only TT pair straddling ref_begin - 1 / ref_begin or ref_end / ref_end + 1 (must not count), a pair
inside the span with an I run between its columns or with a D column on the second T (must count), no T at all.  Every parameter set
of penaltyT x minStability x penaltyC sees the same alignments.

What must hold, restated here from the rule's derivation and not from the header:
  * rule true  =>  the converted record has tri_score < minStability;
  * with penaltyT >= 0 or minStability <= 0 nothing is certain, and neither is it where vmax (nt - 1) + penaltyT < minStability nt - 1
    fails for every nt the spans allow (vmax = max(4.5, penaltyC, 0), 2 <= nt <= 240): the rule is then false for every alignment;
  * length_known  =>  the alignment leaves a record (total >= ntMin)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS = 6000


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """One run of the driver: {(penaltyT, penaltyC, minStability, ntMin, ntMax): {counter: value}} and the strand_miss count."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("doomed") / "doomed_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-misleading-indentation", "-o", exe, os.path.join(ROOT, "tests", "doomed_main.cpp"),
                    os.path.join(ROOT, "fasim-longtarget_amd", "csrc", "host_post.cpp"), "-lpthread"], check=True)
    text = subprocess.run([exe, "12345", str(TRIALS)], check=True, capture_output=True, text=True).stdout
    out, strand_miss = {}, None
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "strand_miss":
            strand_miss = int(f[1])
        else:
            assert f[0] == "set"
            key = (int(f[1]), int(f[2]), float(f[3]), int(f[4]), int(f[5]))
            out[key] = {f[k]: int(f[k + 1]) for k in range(6, len(f), 2)}
    return out, strand_miss


def _can_be_certain(pt, pc, mins):
    if pt >= 0 or mins <= 0:
        return False
    vmax = max(4.5, pc, 0)
    return any(vmax * (nt - 1) + pt < mins * nt - 1 for nt in range(2, 241))


def test_every_parameter_set_ran(rows):
    out, strand_miss = rows
    assert strand_miss == 0
    want = {(pt, pc, s, 20, 100000) for pt in (-1000, -1, 0, 5) for s in (0.0, 1.0, 4.6) for pc in (0, -3, 6)}
    assert want <= set(out) and (-1000, 0, 1.0, 20, 30) in out
    assert all(r["cases"] == TRIALS for r in out.values())


def test_rule_true_means_the_record_fails_the_filter(rows):
    out, _ = rows
    assert {k: r["stab_miss"] for k, r in out.items() if r["stab_miss"]} == {}
    assert {k: r["coord_miss"] for k, r in out.items() if r["coord_miss"]} == {}
    # not vacuous: under the default and its neighbours the rule fires for a good part of the alignments
    for key in ((-1000, 0, 1.0, 20, 100000), (-1000, 6, 4.6, 20, 100000), (-1, 0, 4.6, 20, 100000), (-1000, 0, 1.0, 20, 30)):
        assert out[key]["rule"] > TRIALS // 4, key


def test_rule_false_where_nothing_is_certain(rows):
    out, _ = rows
    for (pt, pc, mins, _ntmin, _ntmax), r in out.items():
        if not _can_be_certain(pt, pc, mins):
            assert r["rule"] == 0, (pt, pc, mins)
    assert out[(-5000, 0, 1.0, 20, 100000)]["rule"] == 0      # beyond the penalties the float argument covers


def test_planted_pairs_and_length(rows):
    out, _ = rows
    assert all(r["kind_miss"] == 0 for r in out.values())
    assert all(r["len_miss"] == 0 and r["len_known"] > 0 for r in out.values())
