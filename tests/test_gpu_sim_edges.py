"""Classic SIM (-F) on the GPU at strip, chunk and node-list edges (csrc/sim.hip): k_sim_forward called directly at 1 ... 200 rows
and 1 ... 257 columns on repeats and homopolymers, whole scans of short records, k_sim_resweep suspended after every line and in both
storage variants (option sim_lds), a scan that hands suspended units from the L2 variant to the LDS variant, and units that re-sweep
with a partial node list.  The expected values are the oracle's (sim_forward_nodes, simscan); test_sim_edges_cpu.py asserts what the
inputs reach (list states, ties, rows of more than 64 events, active units) and ties the host half to the oracle.  Every comparison is
exact equality.  GPU only.

Seen on an MI355X (launches of the forced variant / sim_suspended): c, budget 1: b00 2 326 / 28 473, b05 5 534 / 45 191, b10 5 209 /
65 163, b12 5 432 / 101 421, the same under either variant and with or without check mode; budget 5: 508 / 6 037, 1 328 / 9 980,
1 517 / 17 839, 1 189 / 21 119.  d: sim_resweep_l2 210, sim_resweep_lds 5 329, sim_suspended 255 961, sim_handover 252.  e: e0 249 /
5 217, e1 699 / 8 569, e2 714 / 7 284, e3 450 / 14 813, e4 914 / 30 306.  Two value-only mutations of sim.hip, tried once: evicting the
last instead of the first lowest node in nodes_add fails all five forward tests (122 to 248 of a composition's 149 to 248 full lists
differ, and no other list) and every case of c; stretching the `exc` gap of sweep_chunk by t + 1 fails every case of c."""
import os

import pytest

import helpers
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

SIM_STATS = ("sim_resweep_lds", "sim_resweep_l2", "sim_suspended", "sim_handover")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def engine(mod):
    e = mod.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc(oracle_build):
    return helpers.Oracle(oracle_build)


@pytest.fixture(scope="module")
def expected(oracle_build, tmp_path_factory):
    """(query, record) -> the oracle's records under -lg 10 after the tail filter, made once"""
    tmp = tmp_path_factory.mktemp("simedge")
    return lambda q, dna: helpers.simscan_triplexes(helpers.sim_edge_simscan(oracle_build, tmp, q, dna, 10), 10)


def _params(mod):
    return mod.default_params(classicSim=1, cLength=10)


def _scan(mod, q, dna, sim_lds):
    e = mod.Engine(0)
    e.set_option("sim_lds", sim_lds)
    e.set_query(q)
    try:
        return e.scan(dna, _params(mod))
    finally:
        e.close()


def _sim_stats(st):
    return {k: st[k] for k in SIM_STATS}


def _only_variant(st, sim_lds):
    """the launches are counted in the field of the forced variant alone, and no unit changes variant"""
    mine, other = ("sim_resweep_lds", "sim_resweep_l2") if sim_lds else ("sim_resweep_l2", "sim_resweep_lds")
    return st[mine] > 0 and st[other] == 0 and st["sim_handover"] == 0


# ---- a. the forward sweep, called directly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", helpers.SIM_FWD_COMPOSITIONS)
def test_forward_sweep_at_strip_and_chunk_edges(engine, orc, comp):
    """k_sim_forward against the oracle's first sweep: 9 query lengths x 9 target lengths x 5 thresholds of one composition, the
    targets of a query in calls of 1, 5 and 7 with mixed lengths (tail columns padded, units no multiple of a workgroup's 4)."""
    bad, states = [], {"empty": 0, "partial": 0, "full": 0}
    for m in helpers.SIM_FWD_M:
        q, problems = helpers.sim_forward_problems(orc, comp, m)
        engine.set_query(q)
        for batch in helpers.sim_forward_batches(problems):
            got = engine.sim_forward([t for t, _, _ in batch], [thr for _, _, thr in batch])
            for (t, name, thr), g in zip(batch, got):
                exp = orc.sim_forward_nodes(q, t, thr)
                states[helpers.sim_list_state(exp)] += 1
                if g != exp:
                    bad.append((m, len(t), name, thr, len(g), len(exp)))
    print(f"{comp}: lists {states}, {len(bad)} differ")
    assert not bad, (comp, len(bad), bad[:8])
    assert min(states.values()) > 0


# ---- b. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in helpers.SIM_EDGE_CASES if k.startswith("b")])
def test_scan_of_short_records_equals_simscan(mod, engine, expected, name):
    """fasim_scan with classicSim over one short record: forward sweep, K rounds of re-sweeps and the host half, against `simscan`."""
    q, (dna,) = helpers.sim_edge_case(name)
    engine.set_query(q)
    res = engine.scan(dna, _params(mod))
    exp = expected(q, dna)
    assert len(exp) > 0 and res.triplexes() == exp
    assert res.stats["kernel_launches"][7] > 0 and res.stats["units"] == 48


# ---- c. suspend and resume after every line, both variants ---------------------------------------------------------------------
@pytest.mark.parametrize("check, budget", [(True, 1), (True, 5), (False, 1)])
@pytest.mark.parametrize("sim_lds", [0, 1])
@pytest.mark.parametrize("name", helpers.SIM_SUSPEND_CASES)
def test_resweep_suspended_after_every_line(mod, expected, monkeypatch, name, sim_lds, check, budget):
    """A budget of 1 (and of 5) 64-cell steps per launch suspends every unit after each line of the backward, growing and forward
    phases; the LDS variant then spills and reloads its lines' states for every (m1, n1) that occurs.  In check mode every round's
    node lists equal the host re-sweep's or the scan fails; once more without it, so that the device's own lists feed the host half."""
    q, (dna,) = helpers.sim_edge_case(name)
    if check:
        monkeypatch.setenv("FASIM_SIM_RESWEEP", "check")
    else:
        monkeypatch.delenv("FASIM_SIM_RESWEEP", raising=False)
    monkeypatch.setenv("FASIM_SIM_BUDGET", str(budget))
    res = _scan(mod, q, dna, sim_lds)
    print(f"{name} sim_lds {sim_lds} budget {budget}{' check' if check else ''}: {_sim_stats(res.stats)}")
    assert res.triplexes() == expected(q, dna)
    assert res.stats["sim_suspended"] > 0 and _only_variant(res.stats, sim_lds), res.stats


# ---- d. hand-over under the auto rule ----------------------------------------------------------------------------------------------
def test_suspended_units_change_variant_under_the_auto_rule(mod, expected, monkeypatch):
    """8 records x 48 units in one batch: more than 256 active units, so the first launches take the L2 variant; as units finish, the
    count falls through 256 and the units still suspended are resumed by the LDS variant from the state the other one left."""
    q, recs = helpers.sim_edge_case("d-m64-8rec")
    monkeypatch.setenv("FASIM_SIM_RESWEEP", "check")
    monkeypatch.setenv("FASIM_SIM_BUDGET", "3")
    e = mod.Engine(0)
    e.set_query(q)
    try:
        got = e.scan_records(recs, _params(mod))
        tot = e.last_totals[0]
    finally:
        e.close()
    print(f"d-m64-8rec auto: {_sim_stats(tot)}, units {tot['units']}")
    assert tot["units"] == 8 * 48
    assert tot["sim_resweep_l2"] > 0 and tot["sim_resweep_lds"] > 0 and tot["sim_handover"] > 0 and tot["sim_suspended"] > 0
    for r, dna in enumerate(recs):
        exp = expected(q, dna)
        assert len(exp) > 0 and got[r].triplexes() == exp, r


# ---- e. partial lists entering a re-sweep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_lds", [0, 1])
@pytest.mark.parametrize("name", helpers.SIM_PARTIAL_CASES)
def test_resweep_with_partial_lists(mod, expected, monkeypatch, name, sim_lds):
    """A 20-nt and a 65-nt query against records of 6 ... 16 nt: the forward sweep leaves partial lists, which go through the serial
    addnode path of the re-sweeps (some fill there).  The records are shorter than -ni, so there is no triplex to compare: what checks
    the kernel is check mode, round by round, with a budget of one step."""
    q, (dna,) = helpers.sim_edge_case(name)
    monkeypatch.setenv("FASIM_SIM_RESWEEP", "check")
    monkeypatch.setenv("FASIM_SIM_BUDGET", "1")
    res = _scan(mod, q, dna, sim_lds)
    print(f"{name} sim_lds {sim_lds} budget 1 check: {_sim_stats(res.stats)}")
    assert res.triplexes() == expected(q, dna)
    assert res.stats["units"] == 48 and res.stats["kernel_launches"][7] > 0
    assert res.stats["sim_suspended"] > 0 and _only_variant(res.stats, sim_lds), res.stats
