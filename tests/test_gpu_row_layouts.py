"""Every rows-per-lane build of the systolic kernels.  k_scan (integer, F16, ROWS, ROWS + F16, DUMP) and k_align_fwd (TAINT, word,
REV, REV + F16) are compiled once per RP = 1 ... 24, and the query length alone decides which build runs.  The 48 generated cases
of helpers.row_layout_cases() reach each RP twice: every virtual lane with RP rows, and two lanes of a stripe with RP rows, six with
RP - 1 and 15 pad rows.  test_row_layouts_cpu.py proves on the CPU that each case holds triplexes, units beyond the byte range and
an F >= 132 crossing a stripe boundary.  The oracle scans each case once, live; all comparisons are exact (integer DP).

  a. stages 1 and 2 through the raw call pre_align_batch, unit by unit against the oracle.  That call runs the stripe-faithful
     kernels (k_striped), not k_scan: a changed k_scan leaves it untouched;
  a'. k_scan's own column maxima, f16 and integer main pass: the bin = 1 potential tracks of the rule-1 units against the numpy
     definition (a failure here is k_scan's and nothing else's);
  b. the full scan against the oracle's triplexes;
  c. every switch gives the records of (b): integer kernels, no band, band without reverse passes, whole-unit and chunked hazard
     re-runs (the DUMP build);
  d. the planted windows through align_batch: scores of 251 and more take the 16-bit word build of k_align_fwd;
  the ROWS builds are swept by test_gpu_tfo_profile.test_row_layouts_planted.
GPU only."""
import os

import pytest

import numpy as np

import helpers
import __graft_entry__ as entry
from test_track_cpu import expected_tracks

pytestmark = pytest.mark.gpu

CASES = helpers.row_layout_cases()
SWITCHES = ({"dp_f16": 0}, {"band": 0}, {"band": 2}, {"hazard_chunks": 0}, {"hazard_chunks": 1, "hazard_snapshots": 1},
            {"hazard_chunks": 1, "hazard_chunk_cols": 64})


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def sweep(mod, oracle_build, tmp_path_factory):
    """case -> inputs, the oracle's units and the default scan, each computed once and left unchanged"""
    tmp = tmp_path_factory.mktemp("row_layouts")
    cache = {}
    orc = helpers.Oracle(oracle_build)

    def get(m):
        if m not in cache:
            rna, dna, plants = helpers.row_layout_inputs(m)
            meta, units = helpers.oracle_scan_case(oracle_build, tmp, m)
            assert meta["m"] == m and len(units) == 96
            cache[m] = {"rna": rna, "dna": dna, "plants": plants, "units": units, "base": None, "q2": helpers.q2_units_of_gap_plants(orc, m)}
        return cache[m]

    def base(m):
        c = get(m)
        if c["base"] is None:
            c["base"] = _scan(mod, c["rna"], c["dna"])
        return c["base"]

    get.base = base
    return get


def _scan(mod, rna, dna, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_query(rna)
    r = e.scan(dna, mod.default_params(cLength=20))          # cLength == ntMin: LongTarget's tail filter == fastSIM's
    e.close()
    return r


@pytest.mark.parametrize("dp_f16", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_unit_summaries(mod, sweep, case, dp_f16):
    """(a) (enc, stage-1 maximum, threshold, column-maximum hash, candidate count) of all 96 units against the oracle's U lines
    (the stripe-faithful kernels at this query length; dp_f16 must not matter to them)."""
    k, layout, m = case
    c = sweep(m)
    p = mod.default_params()
    step = p.cutLength - p.overlapLength
    targets = [mod.encode_unit(c["dna"][u["seg"] * step:u["seg"] * step + p.cutLength], u["enc"])[0] for u in c["units"]]
    assert [len(t) for t in targets] == [u["n"] for u in c["units"]]
    e = mod.Engine(0)
    e.set_option("dp_f16", dp_f16)
    e.set_query(c["rna"])
    cols, s1 = e.pre_align_batch(targets)
    e.close()
    hashes = helpers.fnv1a_rows(cols)
    bad = []
    for i, u in enumerate(c["units"]):
        thr = int(s1[i] * 0.8)                      # Fasim-LongTarget.cpp:413
        got = (u["enc"], s1[i], thr, hashes[i], len(mod.pick_candidates(cols[i], thr)))
        exp = (u["enc"], u["stage1"], u["thr"], u["colhash"], u["ncand"])
        if got != exp:
            bad.append((u["seg"], got, exp))
    assert not bad, f"RP {k} {layout} m {m} dp_f16 {dp_f16}: {len(bad)} units differ; (segment, got, oracle) {bad[:3]}"


@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_column_maxima_of_the_scan(mod, case):
    """(a') What k_scan itself computes: under rule 1 (encodings 0, 1, 12, 13, whose units hold exact 32-row hits at a stripe
    boundary) the bin = 1 potential track is, per class, the column maximum of the textbook recurrence, for every base of the
    record.  Exact, against the numpy definition of test_track_cpu, with the f16 and the integer main pass."""
    k, layout, m = case
    rna, dna, _ = helpers.row_layout_inputs(m)
    p = mod.default_params(rule=1, strand=0)
    want, top = expected_tracks(rna, dna, p)
    assert max(top) >= 148
    for f16 in (1, 0):
        e = mod.Engine(0)
        e.set_option("dp_f16", f16)
        e.set_query(rna)
        none, t = e.scan_track(dna, p, bin=1, records=False)
        e.close()
        assert none is None and (t.bin, t.nbins, t.units) == (1, len(dna), 8)
        got = np.asarray(t.array(), dtype=np.int64)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"RP {k} {layout} m {m} dp_f16 {f16}", len(bad), [(int(c), int(x), int(got[c, x]), int(want[c, x])) for c, x in bad[:6]])


@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_full_scan(mod, sweep, case):
    """(b) default options: every triplex of the oracle bit for bit, and the stage-3 paths the case is there for."""
    k, layout, m = case
    c = sweep(m)
    seg = (m + 15) // 16
    res = sweep.base(m)
    st = res.stats
    classes = helpers.band_classes_restated(m)
    print(f"RP {k} {layout} m {m} seg {seg}: hazard_units {st['hazard_units']} (Q2 matters in {len(c['q2'])} units of gapped plants), band classes {classes}, band_tries {st['band_tries']}, "
          f"rev_bound_passes {st['rev_bound_passes']}, align_word_reruns {st['align_word_reruns']}, dp_f16_reruns {st['dp_f16_reruns']}")
    assert st["kernel_launches"][0] > 0
    assert st["units"] == len(c["units"])
    assert st["candidates"] == sum(u["ncand"] for u in c["units"])
    assert res.triplexes() == helpers.expected_triplexes(c["units"])
    if seg < 96:
        assert st["hazard_units"] >= 1            # an F >= 132 crosses a stripe boundary (test_row_layouts_cpu): the unit-level flag
    # every unit in which the reference's signed lazy-F exit changes a column maximum above the threshold (oracle) must have been
    # sent to the stripe-faithful kernels: with seg >= 96 that is the row analysis' doing
    assert st["hazard_units"] >= len(c["q2"])
    if classes:
        assert st["band_tries"] > 0 and st["rev_bound_passes"] > 0     # the REV + F16 build of this RP has run


@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_switches_give_the_same_records(mod, sweep, case):
    """(c) the integer kernels, the band switches and the three hazard re-runs give the records and the pool of (b)."""
    k, layout, m = case
    c = sweep(m)
    base = sweep.base(m)
    assert base.count > 0
    for opts in SWITCHES:
        r = _scan(mod, c["rna"], c["dna"], **opts)
        assert r.stats["kernel_launches"][0] > 0
        assert (r.recs, r.pool) == (base.recs, base.pool), f"RP {k} {layout} m {m}: {opts}"
        assert r.stats["candidates"] == base.stats["candidates"], opts
        if opts == {"dp_f16": 0} and helpers.band_classes_restated(m):
            assert r.stats["band_tries"] > 0 and r.stats["rev_bound_passes"] > 0      # the integer REV build of this RP has run


@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_planted_windows(mod, sweep, oracle_build, case):
    """(d) ssw_align of every plant's window (the plant and ten bases on either side, at most 76 nt) against the oracle: score, both
    ends on both sequences and the CIGAR.  A full scan never sends a window of 251 or more to stage 3 (the overflow cut of stage 2
    hides the columns that could end one), so only here does the 16-bit word build of k_align_fwd run for this RP: the forward
    pass comes back at 251 or more and the window is run again without the byte rules (run_fwd_both)."""
    k, layout, m = case
    c = sweep(m)
    orc = helpers.Oracle(oracle_build)
    # (not the gapped plants: a window that ends in a long vertical gap can send the reference's banded traceback into memory it
    # never wrote, where the oracle has no answer: it reports score 0 and marks the alignment as undefined)
    plants = [p for p in c["plants"] if not p.get("gap")]
    wins = [mod.encode_unit(c["dna"][max(0, p["pos"] - 10):p["pos"] + p["n"] + 10], p["enc"])[0] for p in plants]
    assert max(len(w) for w in wins) <= 200            # longer windows take the striped kernels
    exp = [orc.align(c["rna"], w) for w in wins]
    scores = [five[0] for five, _ in exp]
    print(f"RP {k} {layout} m {m}: window scores {scores}")
    assert sum(s >= 251 for s in scores) >= 2 and sum(148 <= s < 251 for s in scores) >= 2
    e = mod.Engine(0)
    e.set_query(c["rna"])
    got = e.align_batch(wins)
    e.close()
    for a, (five, cig), p in zip(got, exp, plants):
        assert (a.sw_score, a.ref_begin, a.ref_end, a.query_begin, a.query_end) == five and a.cigar_string() == cig, (m, p)
