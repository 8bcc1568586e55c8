"""The inputs of the rows-per-lane sweep (helpers.row_layout_inputs) are the right inputs: the 48 query lengths reach every build
RP = 1 ... 24 of the systolic kernels in both layouts, and the generated DNA drives each case through the paths that the GPU sweep
(test_gpu_row_layouts.py) is about: triplexes and window tries, units beyond the byte range (Q1), an F of 132 or more crossing a
stripe boundary of the reference (Q2), a unit in which that really changes the reference's result where the stripes are long
enough for the row analysis, and all three band-class situations.  Needs no GPU: the oracle and a plain Gotoh only."""
import time

import numpy as np
import pytest

import helpers
from test_track_cpu import _CODE, encode_unit

CASES = helpers.row_layout_cases()


def test_lengths_reach_every_build_in_both_layouts():
    """RP = ceil(seg / vs), seg = ceil(m / 16), vs = 8 * ceil(seg / 192): each RP once with seg % vs == 0 and once without, one
    tile, and the pad rows the two layouts are named for."""
    assert len(CASES) == 48 and len({m for _, _, m in CASES}) == 48
    assert min(m for _, _, m in CASES) == 113 and max(m for _, _, m in CASES) == 3072
    seen = set()
    for k, layout, m in CASES:
        seg, vs, rp = helpers.systolic_layout(m)
        assert vs == 8 and rp == k, (k, layout, m, seg, vs, rp)
        if layout == "full":
            assert m == 128 * k and 16 * seg == m and seg % vs == 0
        else:
            assert 16 * seg - m == 15
            # RP 1 has no ragged layout (seg < 8 is below the smallest systolic query, 113 rows): there the second case differs
            # by its 15 pad rows alone; every other RP has two lanes of a stripe with RP rows and six with RP - 1
            assert seg % vs == (0 if k == 1 else 2)
        seen.add((rp, layout, seg % vs == 0))
    assert seen == {(1, "full", True), (1, "ragged", True)} | {(k, lay, lay == "full") for k in range(2, 25) for lay in ("full", "ragged")}


def test_band_classes_of_the_sweep():
    """No band class, G = 8 alone, G = 8 and 16: all three occur, and nothing else does."""
    got = {m: tuple(helpers.band_classes_restated(m)) for _, _, m in CASES}
    assert set(got.values()) == {(), (8,), (8, 16)}
    assert got[113] == () and got[1024] == (8,) and got[3072] == (8, 16)


def _boundary_f(rna, target, col0, col1, row0, row1, m):
    """Textbook Gotoh (match 5, mismatch -4, gap 16 + 4 per further base, pad rows score 0) over query rows [row0, row1) and target
    columns [col0, col1) alone, every value outside taken as 0.  All operations are monotone, so each value is a lower bound of the
    whole matrix's.  Returns {row: largest F entering that row}, F[i][j] = max(F[i-1][j] - 4, H[i-1][j] - 16)."""
    q = _CODE[np.frombuffer(rna, dtype=np.uint8)]
    t = _CODE[np.frombuffer(target[col0:col1], dtype=np.uint8)]
    nr = row1 - row0
    h_prev, e_prev = [0] * nr, [0] * nr
    best = {}
    for tc in t:
        h, e = [0] * nr, [0] * nr
        f = 0
        for r in range(nr):
            i = row0 + r
            s = 0 if i >= m else (5 if (q[i] == tc and tc < 4) else -4)
            f = max(f - 4, h[r - 1] - 16, 0) if r else 0
            e[r] = max(e_prev[r] - 4, h_prev[r] - 16, 0)
            h[r] = max(0, (h_prev[r - 1] if r else 0) + s, e[r], f)
            best[i] = max(best.get(i, 0), f)
        h_prev, e_prev = h, e
    return best


def hazard_trigger(m):
    """Largest F that the plain Gotoh sees entering the first row of a stripe (row j * seg, j = 1 ... 15), over the windows of the
    case's plants: (F, boundary row, encoding)."""
    rna, dna, plants = helpers.row_layout_inputs(m)
    seg = (m + 15) // 16
    unit = dna[:5000]
    top = (0, None, None)
    for p in plants:
        if p.get("gap"):
            continue
        target = encode_unit(unit, p["enc"])
        c0 = len(unit) - p["pos"] - p["n"] if p["enc"] & 1 else p["pos"]
        row1 = min(16 * seg, max(p["hi"], p["b"] + 1))
        f = _boundary_f(rna, target, max(0, c0 - 4), min(len(unit), c0 + p["n"] + 4), p["lo"], row1, m)
        for row, v in f.items():
            if row % seg == 0 and 1 <= row // seg <= 15 and v > top[0]:
                top = (v, row, p["enc"])
    return top


@pytest.fixture(scope="module")
def scan_seconds():
    times = {}
    yield times
    if times:
        v = sorted(times.values())
        print(f"oracle scan per case: {v[0]:.2f} ... {v[-1]:.2f} s, {sum(v):.1f} s for {len(v)} cases")


@pytest.mark.parametrize("case", CASES, ids=helpers.row_layout_case_id)
def test_case_drives_the_paths(oracle_build, tmp_path, scan_seconds, case):
    k, layout, m = case
    seg = (m + 15) // 16
    t0 = time.time()
    meta, units = helpers.oracle_scan_case(oracle_build, tmp_path, m)
    scan_seconds[m] = time.time() - t0
    assert meta["m"] == m and meta["dna_len"] == 5000 and len(units) == 96
    trips = sum(len(u["triplexes"]) for u in units)
    tries = sum(len(c["tries"]) for u in units for c in u["cands"])
    over = [u["stage1"] for u in units if u["stage1"] >= 251]
    f, row, enc = hazard_trigger(m)
    q2 = helpers.q2_units_of_gap_plants(helpers.Oracle(oracle_build), m)
    print(f"m {m} RP {k} {layout}: seg {seg}, {sum(u['ncand'] for u in units)} candidates, {trips} triplexes, {tries} tries, "
          f"{len(over)} units >= 251 (max {max(u['stage1'] for u in units)}), F {f} into row {row} (encoding {enc}), Q2 matters in the units of encodings {q2}, "
          f"oracle {scan_seconds[m]:.2f} s")
    assert trips >= 5 and tries >= 300
    assert len(over) >= 1                       # the Q1 overflow cut, and the 16-bit word pass of stage 3
    assert f >= 132                             # wakes the row analysis (seg >= 96) or sets the unit-level flag (seg < 96)
    if seg >= 96:
        assert q2                               # and the row analysis must find a unit to re-run: the reference really differs there
