"""The four storage tiers of the stage-3 finish (run_finish: k_finish_lds with 16 KB and 64 KB of LDS, k_finish with 16 KB and 1 MB
of global scratch) and the stripe-faithful replay, window by window on gapped alignments.  A tier that wrongly hands an alignment
on is repaired by the next one, so the results alone cannot show it: Engine.align_batch(paths=True) reports which pass answered, and
helpers.finish_tier_restated says from the oracle's ends and band widths which one must.  test_finish_tiers_cpu.py shows on the CPU
that the windows reach every tier in every score class.  All comparisons are exact.  GPU only."""
import os
import random

import pytest

import helpers
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def cases(mod, oracle_build):
    """m -> (query, census rows, alignments and paths of ONE align_batch call over all windows), each computed once"""
    orc = helpers.Oracle(oracle_build)
    cache = {}

    def get(m):
        if m not in cache:
            q, rows = helpers.finish_tier_census(orc, m)
            e = mod.Engine(0)
            e.set_query(q)
            got, paths = e.align_batch([r["window"] for r in rows], paths=True)
            e.close()
            cache[m] = (q, rows, [_result(a) for a in got], paths)
        return cache[m]

    return get


def _result(a):
    return (a.sw_score, a.ref_begin, a.ref_end, a.query_begin, a.query_end), a.cigar_string()


def _expected(r):
    return (r["ends"], r["cigar"]) if r["ends"][0] else ((0, 0, 0, 0, 0), "")


@pytest.mark.parametrize("m", helpers.FT_LENGTHS)
def test_one_batch_against_the_oracle(cases, m):
    """(a) score, both ends on both sequences and the CIGAR of every window, and the pass that answered it.  More than 128 windows
    in one call: the waves of k_finish_lds hold lanes that leave at different tiers.
    Measured on an MI355X: paths 1: 78, 2: 111, 3: 21, 4: 20, 5: 4 (the many-runs windows), 0: 1 for 1 200 rows and 73 / 125 / 21 / 21 /
    4 / 1 for 3 300.  The many-runs windows are the regression case of run_align's hand-over to k_banded: their ends come from the
    systolic word pass, which knows no begin, and k_banded used to be given the rectangle from (0, 0)."""
    q, rows, got, paths = cases(m)
    assert len(rows) > 128
    count = {t: paths.count(t) for t in range(6)}
    print(f"m {m}: {len(rows)} windows, answered by path {count}")
    bad = [(r["group"], r["script"], r["cigar"], g) for r, g in zip(rows, got) if (g[0] if g[0][0] else (0, 0, 0, 0, 0), g[1]) != _expected(r)]
    assert not bad, (len(bad), bad[:4])
    wrong = [(r["group"], r["cls"], r["script"], r["cigar"], r["bands"], r["tier"], p) for r, p in zip(rows, paths) if p != r["tier"]]
    for x in wrong:
        print("  path differs:", x)
    assert not wrong, (len(wrong), wrong[:6])
    assert min(count[t] for t in (1, 2, 3, 4)) >= 8 and count[5] >= 3 and count[0] == 1


@pytest.mark.parametrize("m", helpers.FT_LENGTHS)
def test_order_and_batch_independence(mod, cases, m):
    """(b) the same windows shuffled, in batches of 63, 64 and 65, and twenty of them alone through ssw_align: the results and the
    paths of (a).  A wrong [cell][lane] slab or pool offset shows here."""
    q, rows, got, paths = cases(m)
    wins = [r["window"] for r in rows]
    e = mod.Engine(0)
    e.set_query(q)
    order = list(range(len(wins)))
    random.Random(1234 + m).shuffle(order)
    g2, p2 = e.align_batch([wins[i] for i in order], paths=True)
    assert [_result(a) for a in g2] == [got[i] for i in order] and p2 == [paths[i] for i in order]
    for size in (63, 64, 65):
        g3, p3 = [], []
        for k in range(0, len(wins), size):
            g, p = e.align_batch(wins[k:k + size], paths=True)
            g3 += [_result(a) for a in g]
            p3 += p
        assert g3 == got and p3 == paths, size
    for i in order[:20]:
        assert _result(e.ssw_align(wins[i])) == got[i], rows[i]["script"]
    e.close()


@pytest.mark.parametrize("m", helpers.FT_LENGTHS)
def test_no_replay_outside_148_to_250(cases, m):
    """(c) below 148 no taint is possible, from 251 on the word pass has no flags, and the reverse pass cannot run out of its 640
    rows at these sizes: only the CIGARs of more than 48 runs may be replayed."""
    q, rows, got, paths = cases(m)
    bad = [(r["group"], r["script"], r["ends"]) for r, p in zip(rows, paths) if p == 5 and r["cls"] != "mid" and r["group"] != "many-runs"]
    assert not bad, bad[:6]


@pytest.mark.parametrize("m", helpers.FT_LENGTHS)
def test_stripe_faithful_replay_agrees(mod, cases, monkeypatch, m):
    """(d) FASIM_ALIGN_V1=1 in a fresh engine: every window takes the replay, and every result is that of (a)."""
    q, rows, got, paths = cases(m)
    monkeypatch.setenv("FASIM_ALIGN_V1", "1")
    e = mod.Engine(0)
    e.set_query(q)
    g, p = e.align_batch([r["window"] for r in rows], paths=True)
    e.close()
    assert p == [5] * len(rows)
    assert [_result(a) for a in g] == got


def test_scan_finish_counts_its_tiers(mod, oracle_build, tmp_path):
    """(e) the scan's own finish: a 10 kb record with the pre-images of 24 gapped windows (helpers.finish_tier_scan_case; the CPU
    test shows that at least 8 become records) against the oracle's scan, record for record; the four tier counters add up to
    something, the 64 KB LDS pass has answered, and band = 0, 1, 2 give the same records and the same counters."""
    orc = helpers.Oracle(oracle_build)
    q, dna, plants = helpers.finish_tier_scan_case(orc)
    meta, units = helpers.finish_tier_oracle_scan(oracle_build, tmp_path, q, dna)
    keys = ("finish_lds16", "finish_lds64", "finish_glob16k", "finish_glob1m")
    seen = []
    for band in (1, 0, 2):
        e = mod.Engine(0)
        e.set_option("band", band)
        e.set_query(q)
        r = e.scan(dna, mod.default_params(cLength=20))
        e.close()
        counts = tuple(r.stats[k] for k in keys)
        print(f"band {band}: {r.count} records, candidates {r.stats['candidates']}, exact replays {r.stats['exact_replays']}, finish tiers {counts}")
        assert r.stats["candidates"] == sum(u["ncand"] for u in units)
        assert r.triplexes() == helpers.expected_triplexes(units), band
        assert sum(counts) > 0 and counts[1] > 0, counts
        seen.append(((r.recs, r.pool), counts))
    assert seen[0] == seen[1] == seen[2]
