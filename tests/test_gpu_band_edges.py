"""The banded forward pass of stage 3 (band.hip: k_band_decide, k_band_emit, k_align_band<8|16|32>) at the edges of its classes,
zones and bounds.  helpers.band_edge_inputs plants alignments below 148 (a window with a bound of 148 or more is never banded)
where a band rule that is off by a lane, or a theta one too small, would change a record: at row 0 and in the last, partly dead
profile lane; across multiples of 48 rows, the zone boundary (row 3 072) and the tile boundary of k_scan; twins that tie hundreds
of rows apart (the reference reports the smaller row); paths made tall by a vertical gap; in the first and last columns of a
segment and in the short tail segment; beside a 160-point plant; beside a longer plant that ends just after the window.  The query
lengths are the smallest at which each band class, zone count and tile count first occurs (test_band_edges_cpu.py pins them and
shows from the oracle that every plant is what it claims).  The oracle scans each case once, live; every comparison is exact.

  records   Engine.scan with band = 1 (default), 2 and 0, with the integer k_scan (dp_f16 = 0) and with seg_batch = 1: the oracle's
            triplexes, units and candidate counts;
  counters  no band try at 1 008 rows or with band = 0; from 1 009 on proven bands, and reverse passes under band = 1 only;
  paths     the `fasim` CLI as a child process with FASIM_BAND_DEBUG=1 (the variable is read once per process): tries of every class
            the layout lists, windows refused for a bound >= 148, windows without a band, second bands, and bands from the bounds
            of a reverse pass all occur, and the child's -TFOsorted file is the in-process text.
GPU only."""
import os
import re
import subprocess

import pytest

import helpers
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

LENGTHS = helpers.BAND_EDGE_LENGTHS
MODES = ({}, {"band": 2}, {"band": 0}, {"dp_f16": 0}, {"seg_batch": 1})
BAND_LINE = re.compile(r"\[band\] pass (\d+): (\d+) tries looked at \((\d+) with bounds of an earlier pass\), classes (\d+) / (\d+) / (\d+), "
                       r"bound >= 148: (\d+), no band: (\d+); after the pass (\d+) of (\d+) proven, (\d+) unproven")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def sweep(oracle_build, tmp_path_factory):
    """m -> the case's files and inputs and the oracle's units, computed once and left unchanged"""
    tmp = tmp_path_factory.mktemp("band_edges")
    cache = {}

    def get(m):
        if m not in cache:
            rna_fa, dna_fa, rna, dna, plants = helpers.band_edge_files(tmp, m)
            meta, units = helpers.parse_scan(helpers.band_edge_oracle_scan(oracle_build, tmp, m, detail=0))
            assert meta["m"] == m and meta["nseg"] == 3 and len(units) == 144
            cache[m] = {"rna_fa": rna_fa, "dna_fa": dna_fa, "rna": rna, "dna": dna, "plants": plants, "units": units, "dir": tmp}
        return cache[m]

    return get


def _params(mod):
    p = mod.default_params(**helpers.scan_option_fields(helpers.SCAN_OPEN))
    p.cLength = p.ntMin          # LongTarget's tail filter == fastSIM's: no record filter can hide a wrong try
    return p


def _scan(mod, c, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_query(c["rna"])
    r = e.scan(c["dna"], _params(mod))
    e.close()
    return r


@pytest.mark.parametrize("opts", MODES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("m", LENGTHS)
def test_records_and_counters(mod, sweep, m, opts):
    c = sweep(m)
    res = _scan(mod, c, **opts)
    st = res.stats
    nl, zs, zones, classes = helpers.band_layout_restated(m)
    print(f"m {m} {opts}: classes {classes}, zones {zones}, band_tries {st['band_tries']}, band_proven {st['band_proven']}, "
          f"rev_bound_passes {st['rev_bound_passes']}, records {res.count}")
    assert st["kernel_launches"][0] > 0
    assert st["units"] == len(c["units"])
    assert st["candidates"] == sum(u["ncand"] for u in c["units"])
    assert res.triplexes() == helpers.expected_triplexes(c["units"])
    assert res.count > 100
    band = opts.get("band", 1)
    if band == 0 or not classes:
        assert st["band_tries"] == 0 and st["band_proven"] == 0 and st["rev_bound_passes"] == 0
    else:
        assert st["band_tries"] > 0 and st["band_proven"] > 0
        assert (st["rev_bound_passes"] > 0) if band == 1 else (st["rev_bound_passes"] == 0)


@pytest.mark.parametrize("m", [m for m in LENGTHS if m >= 1009])
def test_paths_of_a_fresh_process(mod, sweep, m):
    c = sweep(m)
    out = c["dir"] / f"out{m}"
    out.mkdir()
    env = dict(os.environ, FASIM_BAND_DEBUG="1")
    # (file names relative to the working directory: the CLI builds its output names from them)
    cmd = ["timeout", "-k", "10", "120", os.path.join(entry.PKG_DIR, "fasim"), "-f1", os.path.basename(c["dna_fa"]), "-f2", os.path.basename(c["rna_fa"]),
           "-O", f"out{m}/", *helpers.SCAN_OPEN, "-lg", "1", "-ds", "5"]
    child = subprocess.run(cmd, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, cwd=str(c["dir"]))
    assert child.returncode == 0, child.stderr.decode()[-2000:]
    lines = [BAND_LINE.search(x) for x in child.stderr.decode().splitlines() if x.startswith("[band] pass")]
    assert lines and all(lines), "the [band] pass lines of stderr do not parse"
    rows = [tuple(int(x) for x in g.groups()) for g in lines]
    per_class = [sum(r[3 + k] for r in rows) for k in range(3)]
    hot, noband = sum(r[6] for r in rows), sum(r[7] for r in rows)
    second = sum(r[1] for r in rows if r[0] == 1)
    withprev = sum(r[2] for r in rows)
    nl, zs, zones, classes = helpers.band_layout_restated(m)
    print(f"m {m}: tries per class G8 / G16 / G32 {per_class[0]} / {per_class[1]} / {per_class[2]}, bound >= 148 {hot}, no band {noband}, "
          f"second bands looked at {second}, with bounds of an earlier pass {withprev}")
    for k, G in enumerate((8, 16, 32)):
        if G in classes:
            assert per_class[k] > 0, f"m {m}: no try of class G = {G}"
        else:
            assert per_class[k] == 0, f"m {m}: tries of class G = {G}, which the layout does not list"
    assert hot > 0, f"m {m}: no window was refused for a bound >= 148"
    assert noband > 0, f"m {m}: no window was left without a band"
    assert second > 0, f"m {m}: no second band (pass 1)"
    assert withprev > 0, f"m {m}: no try with bounds of an earlier pass"
    files = sorted(f for f in os.listdir(out) if f.endswith("-TFOsorted"))
    assert len(files) == 1, files
    res = _scan(mod, c)
    p = _params(mod)
    p.cDistance = 5              # (the top plant's mid-point is row 12: the reference's clustering needs it at -ds or beyond)
    _, chro, start = mod.parse_dna_header(f"syn|chrB|1-{len(c['dna'])}")
    text = mod.tfosorted(res, chro, start, p)
    assert text.count(b"\n") > 100
    assert (out / files[0]).read_bytes() == text
