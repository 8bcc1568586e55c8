"""The inputs of the band-edge sweep (helpers.band_edge_inputs) are what they claim, shown from the oracle's `scan` (its T lines:
window length L, score, ref_end, q_end, CIGAR) in the manner of test_row_layouts_cpu.py: every plant is a candidate of its unit, the
try that decides it has the planted score (below 148, so the window is one the banded stage 3 may take) and ends at the planted
query row; equal twins end at the upper copy; tall and wide plants hold a gap run of exactly g.  The band layout of the sweep's
query lengths is pinned from the formulas of band.hip written out in helpers.band_layout_restated.  Two cases are tied to the
reference itself (tests/golden/band_m<m>.scan.gz, `make_golden.py band`).  test_gpu_band_edges.py holds the engine to the
oracle's live scan of the same inputs.  Needs no GPU."""
import os
import re

import pytest

import helpers

LENGTHS = helpers.BAND_EDGE_LENGTHS
PINNED = (1009, 4081)


def _first(pred, lo, hi):
    return next(m for m in range(lo, hi) if pred(m))


def test_layout_transitions():
    """The query lengths at which each band class, the second zone (and tile) and the third zone first occur."""
    lay = helpers.band_layout_restated
    assert lay(1008)[3] == [] and lay(1009)[3] == [8]
    assert _first(lambda m: 8 in lay(m)[3], 113, 7000) == 1009
    assert _first(lambda m: 16 in lay(m)[3], 113, 7000) == 2017
    assert _first(lambda m: 32 in lay(m)[3], 113, 7000) == 4081
    assert _first(lambda m: lay(m)[2] == 2, 113, 7000) == 3073
    assert _first(lambda m: helpers.systolic_layout(m)[1] == 16, 113, 7000) == 3073
    assert _first(lambda m: lay(m)[2] == 3, 113, 7000) == 6145
    # below 3 073 rows the restated classes are those of the row-layout sweep's shorter statement
    for m in (113, 1008, 1009, 2016, 2017, 3072):
        assert lay(m)[3] == helpers.band_classes_restated(m), m
    got = {m: lay(m) for m in LENGTHS}
    assert got[1008] == (21, 21, 1, []) and got[1009] == (22, 22, 1, [8]) and got[2017] == (43, 43, 1, [8, 16])
    assert got[3073] == (65, 64, 2, [8, 16]) and got[4081] == (86, 64, 2, [8, 16, 32]) and got[6000] == (125, 64, 2, [8, 16, 32])
    # 1 009 has 15 pad rows; the second tile of 3 073 starts at row 1 544, that of 6 000 at row 3 000, not the zone boundary 3 072
    assert 16 * ((1009 + 15) // 16) - 1009 == 15
    assert 8 * ((3073 + 15) // 16) == 1544 and 8 * ((6000 + 15) // 16) == 3000
    assert helpers.scan_lane_of_row(3073, 1543) == 127 and helpers.scan_lane_of_row(3073, 1544) == 128
    assert helpers.scan_lane_of_row(6000, 2999) == 127 and helpers.scan_lane_of_row(6000, 3000) == 128


def test_plant_kinds_per_length():
    """Every kind at every length where it exists, every plant below 148 but the hot one, distinct names."""
    for m in LENGTHS:
        rna, dna, plants = helpers.band_edge_inputs(m)
        nl, zs, zones, classes = helpers.band_layout_restated(m)
        assert len(rna) == m and len(dna) == helpers.BAND_EDGE_DNA_LEN
        assert set(rna) <= set(b"ACGT") and set(dna) <= set(b"ACGTN")
        assert dna.count(b"N") <= 2 * helpers.BAND_EDGE_FLANK * len(plants)
        names = [p["name"] for p in plants]
        assert len(set(names)) == len(names)
        kinds = {p["kind"] for p in plants}
        want = {"top", "bottom", "lane-edge", "twin", "tall", "wide", "column-edge", "hot", "hot-neighbour"}
        if classes:
            want |= {"loose-neighbour"}
        if m >= 3073:
            want |= {"zone-edge", "tile-edge"}
        assert kinds == want, (m, kinds ^ want)
        for p in plants:
            assert all(0 <= lo < hi <= m for lo, hi in p["rows"]), (m, p)
            assert (p["score"] == 160) if p.get("hot") else (110 <= p["score"] < 148), (m, p)
            assert p["enc"] in helpers.BAND_EDGE_ENCS and helpers.band_edge_unit_columns(p), (m, p)
        assert {p["gap"] for p in plants if p["kind"] == "tall"} == {1, 4, 8, 12, 16}
        assert {p["ins"] for p in plants if p["kind"] == "wide"} == {1, 4, 8}
        for G in classes:       # the last possible band start nl - G and the lane after it
            assert {f"lane-edge-last-start-G{G}", f"lane-edge-past-last-start-G{G}"} & set(names), (m, G)
        twins = {p["name"] for p in plants if p["kind"] == "twin"}
        assert {"twin-96", "twin-432", "near-twin-upper", "near-twin-lower"} <= twins
        assert ("twin-1008" in twins) == (m >= 2017) and ("twin-1728" in twins) == (m >= 3073)
        if m >= 4081:
            assert sum(p["kind"] == "tall" and p["edge"] == 3072 for p in plants) == 5
        # a tall plant starts above and ends below its edge
        for p in plants:
            if p["kind"] in ("tall", "wide"):
                assert p["rows"][0][0] < p["edge"] <= p["rows"][-1][1] - 1 and p["rows"][0][0] < p["edge"], (m, p)
        # neighbours: B starts after A's window ends and ends in the same 64-step block of k_scan (step = column + lane inside the
        # tile) as that window's last column, in B's last lane; the loose B lies more than the tallest band below A
        by = {p["name"]: p for p in plants}
        for a, b in (("hot-neighbour-near", "hot"), ("loose-A", "loose-B")):
            if a not in by:
                continue
            (sa, ca), (sb, cb) = helpers.band_edge_unit_columns(by[a])[0], helpers.band_edge_unit_columns(by[b])[0]
            v = helpers.scan_lane_of_row(m, by[b]["q_end"]) % 128
            assert sa == sb and by[a]["enc"] == by[b]["enc"] and ca < cb - by[b]["n"] + 1, (m, a, b)
            assert (ca + v) // 64 == (cb + v) // 64, (m, a, b, ca, cb, v)
        if classes:
            assert by["loose-B"]["rows"][0][0] - by["loose-A"]["rows"][0][1] > 48 * classes[-1] and by["loose-B"]["score"] > by["loose-A"]["score"]
        assert abs(helpers.band_edge_unit_columns(by["hot-neighbour-far"])[0][1] - helpers.band_edge_unit_columns(by["hot"])[0][1]) > 200
        # column edges: first and last 30 columns of a long segment, the overlap of two segments, the tail segment
        cols = {p["name"]: helpers.band_edge_unit_columns(p) for p in plants if p["kind"] == "column-edge"}
        assert cols["first-columns"] == [(0, 25)] and cols["last-columns"][0] == (1, 4996) and cols["last-columns"][1][0] == 2
        assert [s for s, _ in cols["overlap"]] == [0, 1] and [s for s, _ in cols["tail-segment"]] == [1, 2]
        assert helpers.BAND_EDGE_SEGMENTS[2][1] < 128


@pytest.fixture(scope="module")
def scans(oracle_build, tmp_path_factory):
    """m -> (raw text, units by (segment, encoding), plants) of the oracle's scan with T lines, each computed once"""
    tmp = tmp_path_factory.mktemp("band_edges")
    cache = {}

    def get(m):
        if m not in cache:
            text = helpers.band_edge_oracle_scan(oracle_build, tmp, m, detail=1)
            meta, units = helpers.parse_scan(text)
            assert meta["m"] == m and meta["nseg"] == 3 and len(units) == 144
            cache[m] = (text, {(u["seg"], u["enc"]): u for u in units}, helpers.band_edge_inputs(m)[2])
        return cache[m]

    return get


def _deciding_try(cand):
    """the try fastSIM keeps: the first that reaches the candidate's score, else the best that ends in the window's last column"""
    best = None
    for t in cand["tries"]:
        if t["score"] >= cand["score"]:
            return t
        if t["ref_end"] == t["L"] - 1 and (best is None or t["score"] > best["score"]):
            best = t
    return best


@pytest.mark.parametrize("m", LENGTHS)
def test_plants_are_what_they_claim(scans, m):
    text, units, plants = scans(m)
    bad, lmod = [], set()
    for p in plants:
        for s, col in helpers.band_edge_unit_columns(p):
            u = units[(s, p["enc"])]
            cand = [c for c in u["cands"] if c["pos"] == col]
            if not cand:
                bad.append(f"{p['name']} (segment {s}, encoding {p['enc']}): no candidate at column {col}; unit maximum {u['stage1']}, threshold {u['thr']}")
                continue
            t = _deciding_try(cand[0])
            if t is None:
                bad.append(f"{p['name']} (segment {s}): no try decides the candidate at column {col}")
                continue
            if cand[0]["score"] != p["score"] or t["score"] != p["score"]:
                bad.append(f"{p['name']} (segment {s}): candidate {cand[0]['score']}, try {t['score']}, planted {p['score']}")
            if t["q_end"] != p["q_end"]:
                bad.append(f"{p['name']} (segment {s}): the try ends at row {t['q_end']}, planted {p['q_end']}")
            if t["q_begin"] != p["rows"][0][0]:
                bad.append(f"{p['name']} (segment {s}): the try begins at row {t['q_begin']}, planted {p['rows'][0][0]}")
            if not p.get("hot") and not t["score"] < 148:
                bad.append(f"{p['name']} (segment {s}): score {t['score']} is not below 148")
            runs = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", t["cigar"])]
            gaps = [(n, op) for n, op in runs if op != "M"]
            want = [(p["gap"], "I")] if p["kind"] == "tall" else [(p["ins"], "D")] if p["kind"] == "wide" else []
            if gaps != want:
                bad.append(f"{p['name']} (segment {s}): CIGAR {t['cigar']} holds the gap runs {gaps}, planted {want}")
            if not p.get("hot"):
                lmod.add(t["L"] % 4)
        if p["kind"] == "twin" and p["name"].startswith("twin-"):
            assert p["q_end"] == p["upper"] + 25, p          # equal twins: the reference reports the smaller row
    assert not bad, f"m {m}: " + "; ".join(bad)
    assert lmod == {0, 1, 2, 3}, f"m {m}: window lengths of the plants' tries take L mod 4 in {sorted(lmod)} only"
    hot = units[(0, helpers.BAND_EDGE_HOT_ENC)]
    assert hot["stage1"] >= 148 and max(c["score"] for c in hot["cands"]) >= 148, f"m {m}: the hot-neighbour unit holds no score >= 148"
    assert sum(c["score"] < 148 for c in hot["cands"]) >= 2
    ncand = sum(u["ncand"] for u in units.values())
    ntries = sum(len(c["tries"]) for u in units.values() for c in u["cands"])
    below = sum(c["score"] < 148 for u in units.values() for c in u["cands"])
    print(f"m {m}: {len(plants)} plants, {ncand} candidates ({below} below 148), {ntries} tries, {sum(len(u['triplexes']) for u in units.values())} records")


@pytest.mark.parametrize("m", PINNED)
def test_oracle_scan_equals_the_reference(oracle_build, golden_dir, tmp_path, m):
    """The oracle's live scan (-detail 0) of two cases is the reference's own, unit by unit."""
    live = helpers.band_edge_oracle_scan(oracle_build, tmp_path, m, detail=0)
    gold = helpers.gunzip(os.path.join(golden_dir, f"band_m{m}.scan.gz"))
    lmeta, lunits = helpers.parse_scan(live)
    gmeta, gunits = helpers.parse_scan(gold)
    assert lmeta == gmeta and len(lunits) == len(gunits) == 144
    for a, b in zip(lunits, gunits):
        assert a == b, f"m {m}: segment {b['seg']} encoding {b['enc']} differs from the reference"
    assert live == gold
