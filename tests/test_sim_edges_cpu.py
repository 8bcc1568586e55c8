"""Classic SIM (-F) at strip, chunk and node-list edges, the CPU half.  test_gpu_sim_edges.py runs k_sim_forward and k_sim_resweep
on inputs made of repeats and homopolymers (helpers.sim_forward_inputs, helpers.sim_edge_case) and compares them with the oracle.
Whether such a comparison says anything depends on what the inputs reach: empty, partial and full node lists, rows with more events
than one replay load, nodes tied for the lowest score, units that re-sweep with a partial list, enough active units for the L2
variant.  This file asserts every such property from the oracle alone, prints the census, and shows that the yardstick of the
engine's check mode (the host half, fasim_sim_finish_unit) equals the oracle's simscan on these shapes.  No GPU."""
import os

import pytest

import helpers
import __graft_entry__ as entry


@pytest.fixture(scope="module")
def orc(oracle_build):
    return helpers.Oracle(oracle_build)


def test_forward_cases_reach_empty_partial_and_full_lists(orc):
    """(a) Every composition ends in empty, partial and full lists; the table per composition and threshold is printed.  Each
    composition has a target of 129 columns or more at threshold 0 with more than 64 events in one row (the e0 loop of the
    replay; counted as cells whose letters match, which score 50 or more), and full lists with two or more nodes tied for the
    lowest score.  The targets of a query go in calls of 1, 5 and 7 with mixed lengths."""
    for comp in helpers.SIM_FWD_COMPOSITIONS:
        table = {name: {"empty": 0, "partial": 0, "full": 0} for name in helpers.SIM_FWD_THRESHOLDS}
        tied, wide_rows, sizes, mixed = 0, 0, set(), 0
        for m in helpers.SIM_FWD_M:
            q, problems = helpers.sim_forward_problems(orc, comp, m)
            assert len(q) == m and len(problems) == len(helpers.SIM_FWD_N) * len(helpers.SIM_FWD_THRESHOLDS)
            assert sorted({len(t) for t, _, _ in problems}) == sorted(helpers.SIM_FWD_N)
            for t, name, thr in problems:
                nodes = orc.sim_forward_nodes(q, t, thr)
                table[name][helpers.sim_list_state(nodes)] += 1
                tied += helpers.sim_tied_lowest(nodes) >= 2
                if name == "0" and len(t) >= 129 and len(nodes) == helpers.SIM_K:
                    wide_rows += helpers.sim_row_events_at_least(q, t) > 64
            for b in helpers.sim_forward_batches(problems):
                sizes.add(len(b))
                mixed += len({len(t) for t, _, _ in b}) > 1
        print(f"{comp:12s} " + "  ".join(f"thr {name}: {c['empty']}/{c['partial']}/{c['full']}" for name, c in table.items())
              + f"  (empty/partial/full)  tied-lowest full lists {tied}, targets with a row of > 64 events {wide_rows}")
        for state in ("empty", "partial", "full"):
            assert sum(c[state] for c in table.values()) > 0, (comp, state)
        assert table["100000"]["empty"] == len(helpers.SIM_FWD_M) * len(helpers.SIM_FWD_N)
        assert table["0"]["full"] > 0 and table["near-best"]["partial"] > 0
        assert tied >= 2, comp
        assert wide_rows >= 1, comp
        assert sizes >= {1, 5, 7} and all(s % 4 for s in sizes) and mixed >= 6      # (batches of 5 and 7 always mix lengths)


@pytest.fixture(scope="module")
def census(orc, oracle_build, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("simedge")
    return {name: helpers.sim_edge_census(orc, oracle_build, tmp, name) for name in helpers.SIM_EDGE_CASES}


def test_scan_cases_hold_what_the_gpu_tests_rely_on(census):
    """(b) every end-to-end case has 48 units with full lists among them and records that pass the tail filter; (c) every unit of the
    suspend / resume cases re-sweeps after its first round; (d) all 8 records of the hand-over case have 48 units that re-sweep after
    the first round: 384 active units in the first launch, above the 256 of the LDS rule; (e) every partial-list case has 48 units,
    partial lists among them, and units that enter a re-sweep with a partial list."""
    for name, rows in census.items():
        for r in rows:
            print(f"{name:14s} units {r['units']} empty/partial/full {r['empty']}/{r['partial']}/{r['full']} tied {r['tied']} "
                  f"re-sweeping {r['sweeps']} (partial {r['partial_sweeps']}) X {r['x']} kept {r['kept']}")
    b = [k for k in census if k.startswith("b")]
    assert len(b) == len(helpers.SIM_SCAN_M) * len(helpers.SIM_SCAN_N)
    for name in b:
        (r,) = census[name]
        assert r["units"] == 48 and r["full"] > 0 and r["sweeps"] > 0 and r["kept"] > 0, (name, r)
    assert sum(census[k][0]["tied"] for k in b) > 0
    for name in helpers.SIM_SUSPEND_CASES:
        (r,) = census[name]
        assert r["sweeps"] == 48 and r["full"] == 48, (name, r)
    rows = census["d-m64-8rec"]
    assert len(rows) == 8 and all(r["units"] == 48 and r["sweeps"] == 48 for r in rows) and 8 * 48 > 256
    assert all(r["kept"] > 0 for r in rows)
    assert len(helpers.SIM_PARTIAL_CASES) == 5
    for name in helpers.SIM_PARTIAL_CASES:
        (r,) = census[name]
        assert r["units"] == 48 and r["partial"] >= 1 and r["partial_sweeps"] >= 1, (name, r)
    assert any(census[k][0]["full"] > 0 for k in helpers.SIM_PARTIAL_CASES)      # and lists that fill in the forward sweep beside them


HOST_HALF_CASES = ("b00-m63-n63", "b05-m64-n65", "b10-m65-n129", "b12-m128-n63", "b18-m129-n129", "b23-m200-n300", "d-m64-8rec") \
    + helpers.SIM_PARTIAL_CASES


def test_host_half_equals_simscan_unit_by_unit(orc, oracle_build, tmp_path):
    """fasim_sim_finish_unit (csrc/host_sim.cpp: best node, traceback, resweep_host) fed with the oracle's node lists gives the
    oracle's simscan records for every unit: resweep_host, which the engine's check mode compares the device re-sweeps with, is right
    on these shapes."""
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    mod = entry.load()
    p = mod.default_params(classicSim=1, cLength=10)
    units_checked = records = 0
    for name in HOST_HALF_CASES:
        q, recs = helpers.sim_edge_case(name)
        for dna in recs:
            for u in helpers.simscan_units(helpers.sim_edge_simscan(oracle_build, tmp_path, q, dna)):
                assert u["seg"] == 0 and u["n"] == len(dna)
                t, _ = orc.encode_unit(dna, u["enc"])
                nodes = orc.sim_forward_nodes(q, t, u["thr"])
                got = [x[:13] for x in mod.sim_finish_unit(q, dna, u["enc"], 0, u["thr"], nodes, p).triplexes()]
                assert got == u["x"], (name, u["enc"], len(got), len(u["x"]))
                units_checked += 1
                records += len(got)
    print(f"{units_checked} units, {records} records")
    assert units_checked == 48 * (len(HOST_HALF_CASES) + 7) and records > 1000
