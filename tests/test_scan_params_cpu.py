"""The triplex scan off its default parameters, on the CPU: the oracle (oracle/) against the reference's scans of the cases of
helpers.SCAN_PARAM_PINNED (tests/golden/params_<case>.scan.gz, made by `make_golden.py params`), and what those fixtures must
hold to be worth comparing with.  test_gpu_scan_params.py compares the engine with the same fixtures and, for its live cases, with
the oracle that this file ties to the reference."""
import os
import subprocess

import pytest

import helpers


@pytest.mark.parametrize("name", sorted(helpers.SCAN_PARAM_PINNED))
def test_oracle_scan_equals_the_reference(oracle_build, golden_dir, tmp_path, name):
    case = helpers.SCAN_PARAM_PINNED[name]
    rna_fa, dna_fa = helpers.scan_param_files(golden_dir, tmp_path, name, case)
    out = helpers.oracle_cli(oracle_build, "scan", rna_fa, dna_fa, "-detail", "0", "-threads", "8", *case[2])
    assert out == helpers.gunzip(os.path.join(golden_dir, f"params_{name}.scan.gz"))


def _x_lines(units):
    return [x for u in units for x in u["triplexes"]]


def _default_x_lines(golden_dir):
    return _x_lines(helpers.parse_scan(helpers.gunzip(os.path.join(golden_dir, "planted40k.scan.gz")))[1])


def test_open_filters_multiply_the_records(golden_dir):
    """With the filters open the same units give at least 5 times the records, and every record of the default is among them."""
    default = _default_x_lines(golden_dir)
    _, units = helpers.scan_param_fixture(golden_dir, "open")
    got = _x_lines(units)
    print("open", len(got), "default", len(default))
    assert len(got) >= 5 * len(default)
    for name in helpers.SCAN_PARAM_PINNED:
        _, units = helpers.scan_param_fixture(golden_dir, name)
        print(name, len(_x_lines(units)), "records in", len(units), "units")


@pytest.mark.parametrize("name", helpers.SCAN_THRESHOLD_CASES)
def test_threshold_cases_keep_some_and_drop_some(golden_dir, name):
    default = set(_default_x_lines(golden_dir))
    _, units = helpers.scan_param_fixture(golden_dir, name)
    got = set(_x_lines(units))
    kept, dropped = len(default & got), len(default - got)
    print(name, "keeps", kept, "drops", dropped, "of", len(default))
    assert kept >= 10 and dropped >= 10


def test_threshold_case_needs_both_thresholds(golden_dir):
    """-i 70 -S 2: either threshold alone drops records of the default that the other keeps (identity and mean stability are the
    float fields 9 and 10 of an X line), so that neither can go unread."""
    import struct
    opts = helpers.scan_option_fields(helpers.SCAN_PARAM_PINNED["thresholds"][2])
    vals = [tuple(struct.unpack("f", struct.pack("I", int(x[k], 16)))[0] for k in (9, 10)) for x in _default_x_lines(golden_dir)]
    by_identity = sum(i < opts["minIdentity"] and s >= opts["minStability"] for i, s in vals)
    by_stability = sum(i >= opts["minIdentity"] and s < opts["minStability"] for i, s in vals)
    print("dropped by identity alone", by_identity, "by stability alone", by_stability)
    assert by_identity >= 10 and by_stability >= 10


@pytest.mark.parametrize("name,flag,other", [("pen_stab", "-pc", "-pt"), ("pen_stab_swapped", "-pt", "-pc")])
def test_either_penalty_decides_records(oracle_build, golden_dir, name, flag, other):
    """-S 1 with penalties of -2 and -3: a conversion that read the milder penalty `flag` as the harsher `other` would lose at least
    10 records: the oracle, tied to the fixture above, with `flag` given the value of `other`.  (A record's first eight fields do
    not hold its stability.)  In `pen` (-S -50) the penalties change the stability of a record and never whether it exists."""
    query, dna_file, options = helpers.SCAN_PARAM_PINNED[name]
    opts = list(options)
    assert int(opts[opts.index(flag) + 1]) > int(opts[opts.index(other) + 1])
    opts[opts.index(flag) + 1] = opts[opts.index(other) + 1]
    out = helpers.oracle_cli(oracle_build, "scan", os.path.join(golden_dir, query + ".fa"), os.path.join(golden_dir, dna_file),
                             "-detail", "0", "-threads", "8", *opts)
    wrong = {x[:8] for x in _x_lines(helpers.parse_scan(out)[1])}
    right = {x[:8] for x in _x_lines(helpers.scan_param_fixture(golden_dir, name)[1])}
    print(name, flag, "as", other, ":", len(wrong - right), "records more,", len(right - wrong), "fewer")
    assert len(right - wrong) >= 10


@pytest.mark.parametrize("name", helpers.SCAN_CUT_CASES)
def test_cut_length_cases_hold_records(golden_dir, name):
    meta, units = helpers.scan_param_fixture(golden_dir, name)
    opts = helpers.scan_option_fields(helpers.SCAN_PARAM_PINNED[name][2])
    assert max(u["n"] for u in units) == min(opts["cutLength"], meta["dna_len"])
    assert sum(bool(u["triplexes"]) for u in units) >= 1


def test_pinned_cases_reach_the_paths_they_are_for(golden_dir):
    _, units = helpers.scan_param_fixture(golden_dir, "ntmax")
    nts = [int(x[7]) for x in _x_lines(units)]
    assert nts and max(nts) <= 40 and min(nts) >= 30
    default_nts = [int(x[7]) for x in _default_x_lines(golden_dir)]
    assert sum(nt > 40 for nt in default_nts) >= 10, "ntMax = 40 must cut into what the default keeps"
    _, units = helpers.scan_param_fixture(golden_dir, "open")
    assert min(int(x[7]) for x in _x_lines(units)) < 20, "open filters must keep records below the default ntMin"
    _, units = helpers.scan_param_fixture(golden_dir, "open_q2")
    assert len({u["seg"] for u in units}) == helpers.SCAN_Q2_SEGMENTS


@pytest.mark.parametrize("rule,strand", sorted(helpers.SCAN_RULE_STRAND))
def test_rule_and_strand_select_encodings(oracle_build, golden_dir, rule, strand):
    """The live cases of the GPU file: the oracle's units per segment are the encodings that (rule, strand) enables, and where the
    compiled reference is present it gives the same scan."""
    args = ["scan", os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "planted40k.fa"), "-detail", "0", "-pt", "0",
            "-r", str(rule), "-t", str(strand)]
    out = helpers.oracle_cli(oracle_build, *args, "-threads", "8")
    meta, units = helpers.parse_scan(out)
    assert len(units) == (meta["nseg"] - len(meta["skipped"])) * helpers.SCAN_RULE_STRAND[(rule, strand)]
    assert sum(len(u["triplexes"]) for u in units) > 0
    if helpers.have_ref_probe():
        assert subprocess.run([helpers.REF_PROBE, *args], check=True, stdout=subprocess.PIPE).stdout == out


@pytest.mark.parametrize("rule,strand", helpers.SCAN_NO_ENCODINGS)
def test_no_encodings_give_the_q_line_alone(oracle_build, golden_dir, rule, strand):
    args = ["scan", os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "testDNA.fa"), "-detail", "0", "-r", str(rule), "-t", str(strand)]
    out = helpers.oracle_cli(oracle_build, *args)
    lines = out.decode().splitlines()
    assert len(lines) == 1 and lines[0].startswith("Q ")
    if helpers.have_ref_probe():
        assert subprocess.run([helpers.REF_PROBE, *args], check=True, stdout=subprocess.PIPE).stdout == out


@pytest.mark.parametrize("name", sorted(helpers.SCAN_PARAM_LIVE_CUTS))
def test_live_cut_lengths(oracle_build, golden_dir, name):
    """The two smallest cut lengths are not pinned: the oracle's scan holds records, and equals the reference's where it is present."""
    query, dna_file, options = helpers.SCAN_PARAM_LIVE_CUTS[name]
    args = ["scan", os.path.join(golden_dir, query + ".fa"), os.path.join(golden_dir, dna_file), "-detail", "0", *options]
    out = helpers.oracle_cli(oracle_build, *args, "-threads", "8")
    meta, units = helpers.parse_scan(out)
    opts = helpers.scan_option_fields(options)
    assert max(u["n"] for u in units) == opts["cutLength"]
    assert sum(bool(u["triplexes"]) for u in units) >= 1
    if helpers.have_ref_probe():
        assert subprocess.run([helpers.REF_PROBE, *args], check=True, stdout=subprocess.PIPE).stdout == out
