"""The windows of the finish-tier tests, checked on the CPU (no GPU needed).

run_finish (engine_stage3.cpp) offers every stage-3 alignment to four passes: k_finish_lds with 16 KB and with 64 KB of LDS, k_finish
with 16 KB and with 1 MB of global scratch; each hands on what it cannot hold, and what none holds is replayed on the stripe-faithful
kernels.  A pass that wrongly hands on is repaired by the next one, so records alone cannot tell which pass answered.
test_gpu_finish_tiers.py therefore asserts, window by window, the pass that Engine.align_batch(paths=True) reports.  This file
establishes what it relies on: helpers.finish_tier_windows gives windows that the oracle aligns with a defined answer, with the
planted gaps, and helpers.finish_tier_restated (a plain restatement of the kernels' fit rules, fed with the oracle's ends and band
widths) sends enough of them to every tier in every score class.  Everything is integer and compared for equality."""
import collections

import pytest

import helpers

CLASSES = ("lo", "mid", "hi")


@pytest.fixture(scope="module")
def orc(oracle_build):
    return helpers.Oracle(oracle_build)


@pytest.mark.parametrize("m", helpers.FT_LENGTHS)
def test_windows_reach_every_tier(orc, m):
    q, rows = helpers.finish_tier_census(orc, m)
    assert len(q) == m and len(rows) > 128
    table = collections.Counter((r["group"], r["cls"], r["tier"]) for r in rows)
    print(f"m {m}: {len(rows)} windows; group, score class, restated tier: count")
    for k in sorted(table):
        print(f"  {k[0]:10s} {k[1]:3s} tier {k[2]}: {table[k]}")
    per = collections.Counter((r["tier"], r["cls"]) for r in rows)
    print("  tier x class:", sorted(per.items()))
    print(f"  tier 3 (16 KB global pass): {sum(r['tier'] == 3 for r in rows)} windows, e.g. {[r['cigar'] for r in rows if r['tier'] == 3][:3]}")
    assert all(0 < len(r["window"]) <= helpers.FT_MAX_WINDOW for r in rows)
    # the oracle aligns every window but the one without a match, and every answer is defined
    assert [r["window"] for r in rows if r["ends"][0] == 0] == [helpers.FT_NO_MATCH]
    assert not [r["window"] for r in rows if r["tainted"]]
    # the planted gaps are in the CIGAR, in every window of the one-gap and doubling groups
    def planted(r):
        return all(f"M{k}{op}" in r["cigar"] for op, k in r["script"] if op in "ID")

    def gaps(r):
        return tuple(x for x in r["script"] if x[0] in "ID")

    one = [r for r in rows if r["group"] == "one-gap"]
    assert not [(r["script"], r["cigar"]) for r in one if not planted(r)]
    assert {gaps(r)[0] for r in one} >= {(op, k) for op in "ID" for k in helpers.FT_ONE_GAP} - {("D", 100)}
    dbl = [r for r in rows if r["group"] == "doubling"]
    assert not [(r["script"], r["cigar"], r["bands"]) for r in dbl if not planted(r)]
    # every k in both orders, each with a band that starts at 1 and doubles until it holds the gap.  One exception, at 1 200 rows:
    # below three flanks of 49 or 52 around a 'D' gap of 40 followed by an 'I' gap of 40, the rows that an F of 132 or more reaches
    # cover a whole 75-row stripe wherever the slice lies, so the byte pass flags that window, it is always replayed, and the
    # generator leaves it out
    missing = {((a, k), (b, k)) for a, b in ("ID", "DI") for k in helpers.FT_DOUBLING} - {gaps(r) for r in dbl}
    print("  doubling scripts without a placement:", sorted(missing))
    assert missing == ({(("D", 40), ("I", 40))} if m == 1200 else set()), missing
    for r in dbl:
        k = gaps(r)[0][1]
        want = [1 << i for i in range(10) if 1 << i < 2 * k]             # 1, 2, ... up to the first width >= k
        assert r["bands"][:len(want)] == want and r["bands"] == [1 << i for i in range(len(r["bands"]))], (r["script"], r["cigar"], r["bands"])
    assert max(len(r["bands"]) for r in dbl) >= 7                                        # 1 ... 64 for the gaps of 40
    # ungapped means ungapped
    assert not [(r["script"], r["cigar"]) for r in rows if r["group"] == "ungapped" and ("I" in r["cigar"] or "D" in r["cigar"])]
    # every tier in every score class in which it can be reached, at least 8 windows each; the 1 MB pass in fewer than 64
    for tier, classes in ((1, CLASSES), (2, CLASSES), (3, ("hi",)), (4, ("hi",))):
        for c in classes:
            assert per[(tier, c)] >= 8, (tier, c, per)
    assert sum(r["tier"] == 4 for r in rows) < 64
    # the replay only for the CIGARs of more than 48 runs
    many = [r for r in rows if r["group"] == "many-runs"]
    assert len([r for r in many if r["runs"] > helpers.FT_MAX_RUNS]) >= 3
    assert [r["group"] for r in rows if r["tier"] == 5] == ["many-runs"] * len(many)
    assert max(r["runs"] for r in rows) <= 62                                            # what the replay's traceback holds
    # the band widths on either side of the limits of the two LDS passes (15 and 63); 61 and 62 would take gaps of 60 and 61
    seen = {b for r in rows for b in r["bands"]}
    assert seen >= {13, 14, 15, 16, 63, 64}, sorted(seen)
    # edges: first and last query row, first and last column, one column
    assert any(r["ends"][3] == 0 for r in rows) and any(r["ends"][4] == m - 1 for r in rows)
    assert any(r["ends"][1] == 0 for r in rows) and any(r["ends"][2] == len(r["window"]) - 1 for r in rows)
    assert any(len(r["window"]) == 1 and r["cigar"] == "1M" for r in rows)
    # ties: the tracts give alignments with gaps
    assert sum(("I" in r["cigar"] or "D" in r["cigar"]) for r in rows if r["group"] == "ties") >= 8


def test_restated_rule_on_hand_made_cases():
    """The restatement itself, where the answer can be read off the sizes (no reverse pass: scores 148 ... 250)."""
    q = w = b"A" * 300
    f = helpers.finish_tier_restated
    assert f(q, w, (0, 0, 0, 0, 0), []) == 0
    assert f(q, w, (200, 0, 39, 0, 39), [1]) == 1
    assert f(q, w, (200, 0, 39, 0, 39), [1], runs=49) == 5
    assert f(q, w, (200, 0, 39, 0, 53), [15]) == 2 and f(q, w, (200, 0, 39, 0, 52), [14]) == 1          # 2 b + 4 <= 32
    assert f(q, w, (200, 0, 99, 0, 99), [1, 2, 4, 8, 16]) == 2                                            # doubling past band 14
    assert f(q, w, (200, 0, 199, 0, 120), [80]) == 4                                                      # 161 * 121 cells
    assert f(q, w, (200, 0, 173, 0, 111), [63]) == 3 and f(q, w, (200, 0, 175, 0, 113), [63]) == 4        # 127 * 112 + 12 * 177 <= 16 384 < 127 * 114 + 12 * 179
    assert f(q, w, (200, 0, 168, 0, 107), [62]) == 2                                                      # 2 b + 4 <= 128


def test_scan_case_sends_gapped_alignments_to_the_finish(orc, oracle_build, tmp_path):
    """Input condition of the scan-level GPU case: in the oracle's scan of the record, at least 8 of the 24 planted gapped
    alignments become triplex records, and more are the alignment a candidate ends with (what the scan's finish works on)."""
    q, dna, plants = helpers.finish_tier_scan_case(orc)
    assert len(q) == helpers.FT_SCAN_M and len(dna) == 10000 and len(plants) == 24
    assert all("I" in p["cigar"] or "D" in p["cigar"] for p in plants)
    meta, units = helpers.finish_tier_oracle_scan(oracle_build, tmp_path, q, dna)
    assert meta["m"] == len(q) and meta["nseg"] == 3
    hit = helpers.finish_tier_planted_records(units, plants)
    wide = [t["cigar"] for u in units for c in u["cands"] for t in c["tries"][-1:] if any(int(n) >= 14 for n, op in _runs(t["cigar"]) if op in "ID")]
    print(f"{sum(len(u['triplexes']) for u in units)} records, {len(hit)} of planted alignments: {[p['cigar'] for p in hit]}; "
          f"{len(wide)} candidates end with a gap of 14 or more")
    assert len(hit) >= 8 and len(wide) >= 8


def _runs(cigar):
    import re
    return re.findall(r"(\d+)([MID])", cigar)


def test_random_search_for_the_16_kb_global_pass(orc):
    """Which windows of at most 200 nt reach tier 3?  A bounded random search over the generator's edit grammar (fixed seed, 2 000
    windows on the 1 200-row query: ungapped with replaced rows, one gap, two gaps of opposite kind; gaps of 1 ... 100, flanks of
    15 ... 95, anywhere in the query, byte-pass flags not considered).  A window must miss the 64 KB LDS pass and fit 16 KB.  It
    cannot miss by the direction cells (more than 16 384 of them do not fit a 16 KB slot either) nor by the ring (an F chain of 254
    rows needs a score above 1 000), so every hit must have a band of 63 or more; the search prints what it finds."""
    import synth
    m = 1200
    q = helpers.finish_tier_query(m)
    rng = synth._Rng(97531)
    hits, tiers = [], collections.Counter()
    for _ in range(2000):
        kind = rng.below(5)
        k = 1 + rng.below(100)
        f = [15 + rng.below(81) for _ in range(3)]
        if kind == 0:
            script = [("M", f[0] + f[1])]
        elif kind in (1, 2):
            script = [("M", f[0]), ("ID"[kind - 1], k), ("M", f[1])]
        else:
            ops = "ID" if kind == 3 else "DI"
            script = [("M", f[0]), (ops[0], k), ("M", f[1]), (ops[1], k), ("M", f[2])]
        cols = sum(n for op, n in script if op in "MD")
        rows = sum(n for op, n in script if op in "MI")
        if cols > helpers.FT_MAX_WINDOW - 10:
            continue
        a = 12 + rng.below(m - rows - 24)
        w, i = bytearray(bytes(b"ACGT"[rng.below(4)] for _ in range(rng.below(6)))), a
        for op, n in script:
            if op == "M":
                w += q[i:i + n]
            if op == "D":
                w += bytes(b"ACGT"[rng.below(4)] for _ in range(n))
            i += n if op in "MI" else 0
        for x in range(rng.below(4)):                       # a few replaced bases
            w[rng.below(len(w))] = b"ACGT"[rng.below(4)]
        w = bytes(w) + bytes(b"ACGT"[rng.below(4)] for _ in range(rng.below(6)))
        ends, cig, tainted, bands = orc.align_ex(q, w)
        if ends[0] == 0 or tainted:
            continue
        t = helpers.finish_tier_restated(q, w, ends, bands, sum(c in "MID" for c in cig))
        tiers[t] += 1
        if t == 3:
            hits.append((cig, bands))
    print(f"random search: restated tiers {sorted(tiers.items())}; tier 3: {len(hits)} windows {hits[:12]}")
    assert sum(tiers.values()) > 1000
    assert all(max(b) >= 63 for _, b in hits), hits
