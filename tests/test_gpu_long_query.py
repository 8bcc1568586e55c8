"""Queries longer than 16 systolic tiles (49 152 nt), up to FASIM_MAX_QUERY = 92 256 nt, and the HBM-window variant of the
stripe-faithful kernel that serves them where the LDS-resident one cannot hold the stripes.  GPU only.

Fixtures: tests/golden/make_golden_long.py (longq92k / longq49k x longq_dna.fa).
"""
import glob
import os
import subprocess

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu


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
def long_dna(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "longq_dna.fa"))


def _query(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


@pytest.fixture(scope="module")
def long_scans(mod, engine, golden_dir, long_dna):
    """-lg 20 scans of both long queries over the long-query record (shared by the parity and the coverage tests)."""
    out = {}
    for name in ("longq49k", "longq92k"):
        engine.set_query(_query(golden_dir, name))
        out[name] = engine.scan(long_dna[1], mod.default_params(cLength=20))
    return out


def _gold(golden_dir, name):
    return open(os.path.join(golden_dir, name), "rb").read()


def test_max_query_is_exported(mod):
    assert mod.MAX_QUERY == 92256


@pytest.mark.parametrize("name", ["longq49k", "longq92k"])
def test_long_query_matches_reference(mod, engine, golden_dir, long_dna, long_scans, name):
    """49 153 nt (the first length past 16 tiles) and 92 256 nt (the limit): triplexes equal to the reference probe's at -lg 20,
    the three output files byte-identical to the reference CLI's at -lg 40."""
    hdr, dna = long_dna
    rna = _query(golden_dir, name)
    _, units = helpers.parse_scan(helpers.gunzip(os.path.join(golden_dir, name + ".scan.gz")))
    res = long_scans[name]
    assert res.stats["units"] == len(units)
    assert res.stats["candidates"] == sum(u["ncand"] for u in units)
    assert res.triplexes() == helpers.expected_triplexes(units)
    assert res.stats["kernel_launches"][0] > 0, "the systolic scan kernel must have run"
    assert res.stats["band_tries"] > 0, "stage 3 must have used row bands"
    if name == "longq92k":
        assert res.stats["striped_window_probs"] > 0, "the HBM-window kernel must have run"
    p = mod.default_params(cLength=40)
    engine.set_query(rna)
    res = engine.scan(dna, p)
    _, chro, start = mod.parse_dna_header(hdr)
    assert mod.tfosorted(res, chro, start, p) == _gold(golden_dir, name + "_lg40.TFOsorted")
    for level in (1, 2):
        got = mod.tfoclass(res, level, chro, start, len(dna), name.upper(), p)
        assert got == _gold(golden_dir, f"{name}_lg40.TFOclass{level}")


def test_long_queries_cover_the_stripe_faithful_paths(long_scans):
    """Over the two queries: hazard re-runs (Q2), 16-bit stage-1 re-runs of saturated units and exact reverse passes."""
    for k in ("hazard_units", "stage1_word_reruns", "rev_exact"):
        assert sum(r.stats[k] for r in long_scans.values()) > 0, (k, {n: r.stats[k] for n, r in long_scans.items()})


@pytest.fixture(scope="module")
def long_default(mod, golden_dir, long_dna):
    _, dna = long_dna
    e = mod.Engine(0)
    e.set_query(_query(golden_dir, "longq92k"))
    r = e.scan(dna, mod.default_params(cLength=30))
    e.close()
    return r


@pytest.mark.parametrize("opts,env", [({"band": 0}, {}), ({"band": 1}, {}), ({"band": 2}, {}), ({}, {"FASIM_ALIGN_V1": "1"}),
                                      ({"hazard_chunks": 0}, {}), ({"hazard_chunks": 1}, {})])
def test_switches_agree_on_long_query(mod, golden_dir, long_dna, long_default, monkeypatch, opts, env):
    """92 256 nt: band modes, stage 3 on the stripe-faithful kernels (MODE_ALIGN on the HBM-window variant in both widths) and the
    two organisations of the hazard re-run give the records and pool of the default run."""
    _, dna = long_dna
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = mod.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_query(_query(golden_dir, "longq92k"))
    r = e.scan(dna, mod.default_params(cLength=30))
    e.close()
    assert r.recs == long_default.recs and r.pool == long_default.pool


def test_scan_v1_agrees_on_long_query_slice(mod, golden_dir, long_dna, monkeypatch):
    """Stages 1 and 2 entirely on the HBM-window kernel (FASIM_SCAN_V1) over the last 10 kb (the saturating block included)."""
    _, dna = long_dna
    part = dna[-10000:]
    rna = _query(golden_dir, "longq92k")
    p = mod.default_params(cLength=30)
    e = mod.Engine(0)
    e.set_query(rna)
    base = e.scan(part, p)
    e.close()
    monkeypatch.setenv("FASIM_SCAN_V1", "1")
    e = mod.Engine(0)
    e.set_query(rna)
    slow = e.scan(part, p)
    e.close()
    assert slow.recs == base.recs and slow.pool == base.pool
    assert slow.stats["kernel_launches"][0] == 0 < base.stats["kernel_launches"][0]


def test_forced_window_agrees_on_long_query(mod, golden_dir, long_dna, monkeypatch):
    """49 153 nt: the 8-bit passes fit the LDS-resident kernel; forcing every launch onto the HBM-window kernel gives the same
    records and pool."""
    _, dna = long_dna
    rna = _query(golden_dir, "longq49k")
    p = mod.default_params(cLength=30)
    e = mod.Engine(0)
    e.set_query(rna)
    base = e.scan(dna, p)
    e.close()
    monkeypatch.setenv("FASIM_STRIPED_WINDOW", "1")
    e = mod.Engine(0)
    e.set_query(rna)
    forced = e.scan(dna, p)
    e.close()
    assert forced.recs == base.recs and forced.pool == base.pool
    assert forced.stats["striped_window_probs"] > base.stats["striped_window_probs"]


@pytest.mark.parametrize("query,dna_name,kw,gold", [
    ("h19_100.fa", "h19_100_dna.fa", dict(cLength=25), "h19_100.TFOsorted"),
    ("H19.fa", "q2cat.fa", dict(cLength=40, overlapLength=0), "q2cat.TFOsorted"),
    ("satq.fa", "sat5k.fa", dict(cLength=40), "sat5k.TFOsorted"),
    ("H19.fa", "planted40k.fa", dict(cLength=40), "planted40k.TFOsorted"),
])
def test_window_kernel_reproduces_fixtures(mod, golden_dir, monkeypatch, query, dna_name, kw, gold):
    """Every stage on the stripe-faithful kernels (FASIM_SCAN_V1 / FASIM_ALIGN_V1), all of them on the HBM-window variant: every
    mode in both widths at lengths where the LDS-resident kernel is the known-good comparison."""
    monkeypatch.setenv("FASIM_STRIPED_WINDOW", "1")
    monkeypatch.setenv("FASIM_SCAN_V1", "1")
    monkeypatch.setenv("FASIM_ALIGN_V1", "1")
    rna = synth.read_fasta(os.path.join(golden_dir, query))[1]
    hdr, dna = synth.read_fasta(os.path.join(golden_dir, dna_name))
    e = mod.Engine(0)
    e.set_query(rna)
    p = mod.default_params(**kw)
    res = e.scan(dna, p)
    e.close()
    _, chro, start = mod.parse_dna_header(hdr)
    assert mod.tfosorted(res, chro, start, p) == _gold(golden_dir, gold)
    assert res.stats["striped_window_probs"] > 0 and res.stats["kernel_launches"][0] == 0


def test_window_kernel_raw_calls_against_oracle(mod, golden_dir, long_dna, oracle_build):
    """calc_score_once and ssw_pre_align of the 92 256-nt query on two 5 kb encoded units, one of which saturates the 8-bit
    pass, against the CPU oracle."""
    _, dna = long_dna
    rna = _query(golden_dir, "longq92k")
    _, units = helpers.parse_scan(helpers.gunzip(os.path.join(golden_dir, "longq92k.scan.gz")))
    sat = max(units, key=lambda u: u["stage1"])
    plain = next(u for u in units if 0 < u["stage1"] < 200 and u["n"] >= 4000)
    orc = helpers.Oracle(oracle_build)
    e = mod.Engine(0)
    e.set_query(rna)
    for u in (sat, plain):
        t, _ = mod.encode_unit(dna[u["dna_start"]:u["dna_start"] + 5000], u["enc"])
        want = orc.stage1_max(rna, t)
        assert e.calc_score_once(t) == want
        assert e.ssw_pre_align(t) == orc.pre_align(rna, t)
    assert orc.stage1_max(rna, mod.encode_unit(dna[sat["dna_start"]:sat["dna_start"] + 5000], sat["enc"])[0]) > 16383
    e.close()


def test_multi_query_batch_with_long_query(mod, engine, golden_dir, long_dna):
    _, dna = long_dna
    qs = [_query(golden_dir, "H19"), _query(golden_dir, "longq92k"), _query(golden_dir, "NEAT1")]
    p = mod.default_params(cLength=40)
    multi = engine.scan_queries(qs, dna, p)
    for q, r in zip(qs, multi):
        engine.set_query(q)
        single = engine.scan(dna, p)
        assert r.recs == single.recs and r.pool == single.pool


def test_cli_long_query(golden_dir, tmp_path):
    exe = os.path.join(entry.PKG_DIR, "fasim")
    for f in ("longq92k.fa", "longq_dna.fa"):
        (tmp_path / f).write_bytes(_gold(golden_dir, f))
    (tmp_path / "out").mkdir()
    subprocess.run([exe, "-f1", "longq_dna.fa", "-f2", "longq92k.fa", "-O", "out/", "-lg", "40"], cwd=tmp_path, check=True,
                   stdout=subprocess.DEVNULL)
    (sorted_file,) = glob.glob(str(tmp_path / "out" / "*-TFOsorted"))
    assert open(sorted_file, "rb").read() == _gold(golden_dir, "longq92k_lg40.TFOsorted")
    for level in (1, 2):
        (f,) = glob.glob(str(tmp_path / "out" / f"*-TFOclass{level}-*"))
        assert open(f, "rb").read() == _gold(golden_dir, f"longq92k_lg40.TFOclass{level}")


def test_query_over_the_limit_is_refused(mod, engine, golden_dir, long_dna, tmp_path):
    _, dna = long_dna
    too_long = _query(golden_dir, "longq92k") + b"A"
    with pytest.raises(mod.FasimError, match="92256"):
        engine.set_query(too_long)
    with pytest.raises(mod.FasimError, match="92256"):
        engine.scan_queries([_query(golden_dir, "H19"), too_long], dna, mod.default_params())
    synth.write_fasta(str(tmp_path / "long.fa"), "TOOLONG", too_long)
    (tmp_path / "dna.fa").write_bytes(_gold(golden_dir, "longq_dna.fa"))
    exe = os.path.join(entry.PKG_DIR, "fasim")
    r = subprocess.run([exe, "-f1", "dna.fa", "-f2", "long.fa", "-O", "out/"], cwd=tmp_path, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE)
    assert r.returncode == 1
    assert b"92256" in r.stderr and b"TOOLONG" in r.stderr
    assert not (tmp_path / "out").exists() or not os.listdir(tmp_path / "out")


def test_classic_sim_limit_unchanged(mod, golden_dir, long_dna):
    """-F keeps its own limit of 65 534 nt (16-bit start fields)."""
    _, dna = long_dna
    e = mod.Engine(0)
    e.set_query(_query(golden_dir, "longq92k")[:65535])
    with pytest.raises(mod.FasimError, match="16 bits"):
        e.scan(dna[:6000], mod.default_params(classicSim=1))
    e.close()
