"""The triplex scan (engine.scan, `fasim -f1 ... -f2 ...`) with its record filters open and its parameters off their defaults,
against the reference's scans of the same cases (tests/golden/params_<case>.scan.gz) and, for the live cases, against the oracle.
test_scan_params_cpu.py ties the oracle to the reference at these parameters and states what the fixtures hold.  GPU only.

cLength is set equal to ntMin everywhere, so that LongTarget's tail filter equals fastSIM's."""
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


def _query(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _params(mod, options, **kw):
    """Parameters of a case: its options, and cLength = ntMin unless the options or kw set it."""
    fields = helpers.scan_option_fields(options)
    fields.update(kw)
    p = mod.default_params(**fields)
    if "cLength" not in fields:
        p.cLength = p.ntMin
    return p


def _assert_scan_equals(res, units):
    assert res.triplexes() == helpers.expected_triplexes(units)
    assert res.stats["units"] == len(units)
    assert res.stats["candidates"] == sum(u["ncand"] for u in units)


def _oracle_units(oracle_build, rna_fa, dna_fa, options):
    out = helpers.oracle_cli(oracle_build, "scan", rna_fa, dna_fa, "-detail", "0", "-threads", "8", *options)
    return helpers.parse_scan(out)


@pytest.mark.parametrize("name", sorted(helpers.SCAN_PARAM_PINNED))
def test_pinned_cases_match_the_reference(mod, engine, golden_dir, name):
    """Every record of the reference's fastSIM() at the case's parameters, unit by unit, identity and stability as float bits."""
    query, dna_file, options = helpers.SCAN_PARAM_PINNED[name]
    _, dna = helpers.scan_param_dna(golden_dir, name, dna_file)
    meta, units = helpers.scan_param_fixture(golden_dir, name)
    engine.set_query(_query(golden_dir, query))
    p = _params(mod, options)
    res = engine.scan(dna, p)
    _assert_scan_equals(res, units)
    assert res.stats["segments"] == meta["nseg"] == mod.segment_count(len(dna), p)
    if name == "open_q2":
        assert res.stats["hazard_units"] > 0


@pytest.mark.parametrize("name", sorted(helpers.SCAN_PARAM_LIVE_CUTS))
def test_small_cut_lengths_match_the_oracle(mod, engine, golden_dir, oracle_build, name):
    """Segments of 64 nt (shorter than the scan's 128-step skew and than one 64-step block) and of 777 nt every 444 (the stride of
    a unit is not its length, and a base lies in two segments)."""
    query, dna_file, options = helpers.SCAN_PARAM_LIVE_CUTS[name]
    rna_fa, dna_fa = os.path.join(golden_dir, query + ".fa"), os.path.join(golden_dir, dna_file)
    meta, units = _oracle_units(oracle_build, rna_fa, dna_fa, options)
    engine.set_query(_query(golden_dir, query))
    p = _params(mod, options)
    res = engine.scan(synth.read_fasta(dna_fa)[1], p)
    _assert_scan_equals(res, units)
    assert res.stats["segments"] == meta["nseg"]


@pytest.mark.parametrize("rule,strand", sorted(helpers.SCAN_RULE_STRAND))
def test_rule_and_strand_match_the_oracle(mod, engine, golden_dir, oracle_build, rule, strand):
    options = ("-pt", "0", "-r", str(rule), "-t", str(strand))
    rna_fa, dna_fa = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "planted40k.fa")
    meta, units = _oracle_units(oracle_build, rna_fa, dna_fa, options)
    engine.set_query(_query(golden_dir, "H19"))
    res = engine.scan(synth.read_fasta(dna_fa)[1], _params(mod, options))
    _assert_scan_equals(res, units)
    assert len(units) > 0 and sum(len(u["triplexes"]) for u in units) > 0
    assert res.stats["units"] == (meta["nseg"] - len(meta["skipped"])) * helpers.SCAN_RULE_STRAND[(rule, strand)]


@pytest.mark.parametrize("rule,strand", helpers.SCAN_NO_ENCODINGS)
def test_no_encodings_give_an_empty_result(mod, engine, golden_dir, oracle_build, rule, strand):
    """A rule that the strand does not have (or that does not exist) enables no encoding: the reference prints its Q line and nothing
    else; the engine returns an empty result without an error and launches no kernel."""
    options = ("-r", str(rule), "-t", str(strand))
    rna_fa, dna_fa = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "testDNA.fa")
    meta, units = _oracle_units(oracle_build, rna_fa, dna_fa, options)
    assert units == []
    hdr, dna = synth.read_fasta(dna_fa)
    engine.set_query(_query(golden_dir, "H19"))
    p = _params(mod, options)
    res = engine.scan(dna, p)            # a return code other than 0 raises FasimError
    assert res.count == 0 and res.triplexes() == [] and res.recs == b""
    assert res.stats["units"] == 0 and res.stats["candidates"] == 0
    assert not any(res.stats["kernel_launches"]), res.stats["kernel_launches"]
    _, chro, start = mod.parse_dna_header(hdr)
    assert mod.tfosorted(res, chro, start, p) == helpers.oracle_cli(oracle_build, "tfosorted", rna_fa, dna_fa, *options, "-lg", "20")


def test_switches_agree_under_open_filters(mod, golden_dir):
    """The integer kernels, the band modes, the whole-unit hazard re-run, the HBM-window striped kernels and Q2 tracking past the
    overflow cut give the records of the default engine also where the filters hide none of them."""
    query, dna_file, options = helpers.SCAN_PARAM_PINNED["open"]
    _, dna = helpers.scan_param_dna(golden_dir, "open", dna_file)
    _, units = helpers.scan_param_fixture(golden_dir, "open")
    rna = _query(golden_dir, query)
    p = _params(mod, options)
    results = []
    for opts in ({}, {"dp_f16": 0}, {"band": 0}, {"band": 2}, {"hazard_chunks": 0}, {"striped_window": 1}, {"q2_past_cut": 1}):
        e = mod.Engine(0)
        for k, v in opts.items():
            e.set_option(k, v)
        e.set_query(rna)
        r = e.scan(dna, p)
        results.append((r.recs, r.pool))
        if not opts:
            assert r.triplexes() == helpers.expected_triplexes(units)
        e.close()
    for k in range(1, len(results)):
        assert results[k] == results[0], k


def test_shards_agree_at_another_cut_length(mod, engine, golden_dir):
    """Segments of 12 345 nt every 10 345 as three contiguous shards, merged in order: the whole scan."""
    query, dna_file, options = helpers.SCAN_PARAM_PINNED["cut12345"]
    _, dna = helpers.scan_param_dna(golden_dir, "cut12345", dna_file)
    _, units = helpers.scan_param_fixture(golden_dir, "cut12345")
    engine.set_query(_query(golden_dir, query))
    p = _params(mod, options)
    whole = engine.scan(dna, p)
    nseg = mod.segment_count(len(dna), p)
    assert nseg >= 3
    cuts = [0, nseg // 3, 2 * nseg // 3, nseg]
    parts = [engine.scan(dna, p, cuts[i], cuts[i + 1] - cuts[i]) for i in range(3)]
    assert all(part.stats["units"] > 0 for part in parts)
    merged = mod.merge_results(parts)
    assert merged.recs == whole.recs and merged.pool == whole.pool
    assert merged.triplexes() == helpers.expected_triplexes(units)


def _oracle_texts(oracle_build, rna_fa, dna_fa, options):
    """(-TFOsorted, -TFOclass1, -TFOclass2) of the oracle, its three runs side by side."""
    exe = os.path.join(oracle_build, "fasim_oracle")
    cmds = [[exe, "tfosorted", rna_fa, dna_fa, "-threads", "5", *options]]
    cmds += [[exe, "tfoclass", rna_fa, dna_fa, "-level", str(level), "-threads", "5", *options] for level in (1, 2)]
    procs = [subprocess.Popen(c, stdout=subprocess.PIPE) for c in cmds]
    outs = [pr.communicate()[0] for pr in procs]
    assert all(pr.returncode == 0 for pr in procs)
    return outs


@pytest.mark.parametrize("name,tail", [("open", ("-lg", "25", "-ds", "5")), ("ntmax", ("-lg", "30", "-ds", "40"))])
def test_text_outputs_match_the_oracle(mod, engine, golden_dir, oracle_build, name, tail):
    """-TFOsorted and both bedGraph files from records that the default filters would hide, at a cluster distance and length of
    their own."""
    query, dna_file, options = helpers.SCAN_PARAM_PINNED[name]
    rna_fa, dna_fa = os.path.join(golden_dir, query + ".fa"), os.path.join(golden_dir, dna_file)
    hdr, dna = synth.read_fasta(dna_fa)
    _, chro, start = mod.parse_dna_header(hdr)
    engine.set_query(_query(golden_dir, query))
    p = _params(mod, options + tail)
    assert (p.cLength, p.cDistance) == (int(tail[1]), int(tail[3]))
    res = engine.scan(dna, p)
    exp = _oracle_texts(oracle_build, rna_fa, dna_fa, options + tail)
    assert exp[0].count(b"\n") > 10
    assert mod.tfosorted(res, chro, start, p) == exp[0]
    for level in (1, 2):
        assert mod.tfoclass(res, level, chro, start, len(dna), query, p) == exp[level], level


def test_cli_reads_every_parameter_flag(golden_dir, oracle_build, tmp_path):
    """`fasim` with every record parameter off its default, -pt != -pc and -ni != -na, so that a swapped pair of flag letters
    shows: the file it writes is the oracle's -TFOsorted text for the same options."""
    exe = os.path.join(entry.PKG_DIR, "fasim")
    for f in ("H19.fa", "planted40k.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    (tmp_path / "out").mkdir()
    options = ["-pt", "-3", "-pc", "-2", "-S", "-50", "-i", "50", "-ni", "25", "-na", "60", "-c", "12345", "-o", "2000", "-lg", "25"]
    oracle = subprocess.Popen([os.path.join(oracle_build, "fasim_oracle"), "tfosorted", str(tmp_path / "H19.fa"), str(tmp_path / "planted40k.fa"),
                               "-threads", "8", *options], stdout=subprocess.PIPE)
    try:
        subprocess.run([exe, "-f1", "planted40k.fa", "-f2", "H19.fa", "-O", "out/", *options], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL)
    finally:
        exp = oracle.communicate()[0]
    assert oracle.returncode == 0
    files = sorted(f for f in os.listdir(tmp_path / "out") if f.endswith("-TFOsorted"))
    assert files == ["syn-H19-planted40k-TFOsorted"]
    assert exp.count(b"\n") > 10
    assert (tmp_path / "out" / files[0]).read_bytes() == exp
