"""The CPU restatement (oracle/) against the reference's own outputs (tests/golden/, made by
tests/golden/make_golden.py from the compiled reference).  CPU only; pins the oracle."""
import os

import pytest

import helpers
import synth


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_demo_scan_identical(oracle_build, golden_dir):
    out = helpers.oracle_cli(oracle_build, "scan", os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "testDNA.fa"))
    assert out == helpers.gunzip(os.path.join(golden_dir, "demo.scan.gz"))


@pytest.mark.parametrize("name,opts", [
    ("demo_lg40.TFOsorted", ["-lg", "40"]),
    ("demo_default.TFOsorted", []),
    ("demo_t1_r3.TFOsorted", ["-lg", "30", "-t", "1", "-r", "3"]),
])
def test_demo_tfosorted_identical(oracle_build, golden_dir, name, opts):
    out = helpers.oracle_cli(oracle_build, "tfosorted", os.path.join(golden_dir, "H19.fa"),
                             os.path.join(golden_dir, "testDNA.fa"), *opts)
    assert out == open(os.path.join(golden_dir, name), "rb").read()


@pytest.mark.parametrize("stem,dna_name,opts", [
    ("demo_lg40", "testDNA.fa", ["-lg", "40"]),
    ("demo_default", "testDNA.fa", []),
    ("demo_t1_r3", "testDNA.fa", ["-lg", "30", "-t", "1", "-r", "3"]),
    ("planted40k", "planted40k.fa", ["-lg", "40"]),
    ("q2cat", "q2cat.fa", ["-o", "0", "-lg", "40"]),
])
def test_tfoclass_bedgraph_identical(oracle_build, golden_dir, stem, dna_name, opts):
    """print_cluster (Fasim-LongTarget.cpp:694): both bedGraph files the reference CLI wrote next to the -TFOsorted file."""
    for level in (1, 2):
        out = helpers.oracle_cli(oracle_build, "tfoclass", os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, dna_name),
                                 "-level", str(level), "-threads", "8", *opts)
        assert out == open(os.path.join(golden_dir, f"{stem}.TFOclass{level}"), "rb").read()


def test_planted40k_scan_and_tfosorted(oracle_build, golden_dir):
    rna, dna = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "planted40k.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-threads", "8")
    gold = helpers.gunzip(os.path.join(golden_dir, "planted40k.scan.gz"))
    assert out == gold
    _, units = helpers.parse_scan(gold)
    assert sum(u["stage1"] >= 251 for u in units) >= 20, "fixture must exercise the byte-overflow (Q1) path"
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "40", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "planted40k.TFOsorted"), "rb").read()


def test_rnd30k(oracle_build, golden_dir, tmp_path):
    dna = _write(tmp_path, "rnd30k.fa", b">syn|chrS|1-30000\n" + synth.random_dna(30000, 12345) + b"\n")
    rna = os.path.join(golden_dir, "H19.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8")
    assert out == helpers.gunzip(os.path.join(golden_dir, "rnd30k.scan.gz"))
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "40", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "rnd30k.TFOsorted"), "rb").read()


def test_batch_vectors(oracle_build, golden_dir):
    o = helpers.Oracle(oracle_build)
    reqs = open(os.path.join(golden_dir, "batch.req")).read().splitlines()
    rsps = open(os.path.join(golden_dir, "batch.rsp")).read().splitlines()
    assert len(reqs) == len(rsps)
    kinds = set()
    for rq, rs in zip(reqs, rsps):
        f, g = rq.split(" "), rs.split(" ")
        q, t = f[1].encode(), f[2].encode()
        kinds.add(f[0])
        if f[0] == "S":
            assert o.stage1_max(q, t) == int(g[1]), rq[:80]
        elif f[0] == "P":
            assert o.pre_align(q, t) == [int(x) for x in g[2:]], rq[:80]
        elif f[0] == "K":
            cands = o.candidates(o.pre_align(q, t), int(f[3]))
            flat = [int(x) for x in g[2:]]
            assert cands == list(zip(flat[0::2], flat[1::2])), rq[:80]
        elif f[0] == "A":
            five, cig = o.align(q, t)
            exp = tuple(int(x) for x in g[1:6])
            if exp[0] == 0:
                assert five[0] == 0
            else:
                assert five == exp and (cig or "*") == g[6], rq[:80]
    assert kinds == {"S", "P", "K", "A"}


def test_q2_units_fixture(oracle_build, golden_dir):
    """19 whole segments, each holding a unit where the signed lazy-F exit (Q2) changes the column maxima."""
    rna, dna = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "q2cat.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-o", "0", "-detail", "0", "-threads", "8")
    assert out == helpers.gunzip(os.path.join(golden_dir, "q2cat.scan.gz"))
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-o", "0", "-lg", "40", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "q2cat.TFOsorted"), "rb").read()
    # the fixture really contains Q2 units: the unsigned-exit variant of the oracle gives different columns
    import ctypes
    o = helpers.Oracle(oracle_build)
    o.lib.fo_pre_align_noq2.restype = None
    o.lib.fo_pre_align_noq2.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    _, q = synth.read_fasta(rna)
    _, d = synth.read_fasta(dna)
    t, _ = o.encode_unit(d[:5000], 44)
    b = (ctypes.c_int * len(t))()
    o.lib.fo_pre_align_noq2(q, len(q), t, len(t), b)
    assert o.pre_align(q, t) != list(b)


@pytest.mark.parametrize("name", ["meg3", "malat1"])
def test_long_queries(oracle_build, golden_dir, name):
    """The reference's example lncRNAs MEG3 (1 582 nt) and MALAT1 (8 708 nt) against planted synthetic DNA."""
    rna = os.path.join(golden_dir, name.upper() + ".fa")
    dna = os.path.join(golden_dir, name + "_dna.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8")
    assert out == helpers.gunzip(os.path.join(golden_dir, name + ".scan.gz"))
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "40", "-threads", "8")
    assert out == open(os.path.join(golden_dir, name + ".TFOsorted"), "rb").read()


def test_stage1_score_beyond_16383(oracle_build, golden_dir):
    """A unit whose exact stage-1 score is 19 905 (only the 16-bit pass of calc_score_once can hold it)."""
    rna, dna = os.path.join(golden_dir, "satq.fa"), os.path.join(golden_dir, "sat5k.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8")
    gold = helpers.gunzip(os.path.join(golden_dir, "sat5k.scan.gz"))
    assert out == gold
    _, units = helpers.parse_scan(gold)
    assert max(u["stage1"] for u in units) > 16383
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "40", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "sat5k.TFOsorted"), "rb").read()


@pytest.mark.parametrize("name", ["h19_700", "h19_100"])
def test_short_queries(oracle_build, golden_dir, name):
    rna, dna = os.path.join(golden_dir, name + ".fa"), os.path.join(golden_dir, name + "_dna.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8")
    assert out == helpers.gunzip(os.path.join(golden_dir, name + ".scan.gz"))
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "25", "-threads", "8")
    assert out == open(os.path.join(golden_dir, name + ".TFOsorted"), "rb").read()


def test_untidy_input(oracle_build, golden_dir):
    """N runs (one whole segment is skipped), lower-case letters and IUPAC codes in the DNA."""
    rna, dna = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "messy.fa")
    out = helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8")
    gold = helpers.gunzip(os.path.join(golden_dir, "messy.scan.gz"))
    assert out == gold
    meta, _ = helpers.parse_scan(gold)
    assert meta["skipped"], "fixture must contain a skipped all-N segment"
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "30", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "messy.TFOsorted"), "rb").read()


# ---- row f3: the -F path (classic SIM, sim.h:410-1143) ------------------------------------------------------------------
def test_classic_sim_demo_units_identical(oracle_build, golden_dir):
    """oracle `simscan` (oracle/fasim_sim_oracle.cpp) against the reference's own SIM() for all 48 units of the demo:
    stage-1 score, threshold and every triplex (coordinates, nt, score, identity / stability as float bits, both strings)."""
    out = helpers.oracle_cli(oracle_build, "simscan", os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "testDNA.fa"), "-threads", "8")
    gold = helpers.gunzip(os.path.join(golden_dir, "demoF.simscan.gz"))
    assert out == gold
    assert gold.count(b"\nX ") > 500


def test_classic_sim_planted12k_identical(oracle_build, golden_dir, tmp_path):
    _, rna = synth.read_fasta(os.path.join(golden_dir, "H19.fa"))
    dna = _write(tmp_path, "simF12k.fa", b">syn|chrF|1-12000\n" + synth.planted_dna(12000, 909, rna, every=700) + b"\n")
    out = helpers.oracle_cli(oracle_build, "simscan", os.path.join(golden_dir, "H19.fa"), dna, "-threads", "8")
    assert out == helpers.gunzip(os.path.join(golden_dir, "simF12k.simscan.gz"))


def test_classic_sim_cli_files_identical(oracle_build, golden_dir):
    """`fasim_ref -F -lg 40` on the demo: -TFOsorted and both -TFOclass files from the oracle's -F path."""
    rna, dna = os.path.join(golden_dir, "H19.fa"), os.path.join(golden_dir, "testDNA.fa")
    out = helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-lg", "40", "-F", "1", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "demoF_lg40.TFOsorted"), "rb").read()
    out = helpers.oracle_cli(oracle_build, "tfoclass", rna, dna, "-lg", "40", "-F", "1", "-level", "1", "-threads", "8")
    assert out == open(os.path.join(golden_dir, "demoF_lg40.TFOclass1"), "rb").read()


# ---- the reference's real DNA: 532 MEG3 ChIP peaks x MEG3 / H19 / MALAT1 (`make_golden.py peaks`) ---------------------------
@pytest.fixture(scope="module")
def peaks(golden_dir):
    return helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))


def _peak_detail(golden_dir, query):
    scans = helpers.split_sections(helpers.gunzip(os.path.join(golden_dir, f"peaks_{query}.detail.scan.gz")))
    files = helpers.split_sections(helpers.gunzip(os.path.join(golden_dir, f"peaks_{query}.detail.files.gz")))
    return {i: s for (i, _), s in scans.items()}, files


@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_peaks_manifest_and_detail_digests(golden_dir, peaks, query):
    """The manifest has one line per record of the reference's DNA file (headers and lengths as stored), and the selected
    records stored in full hash to the manifest's digests: line counts and SHA-256 of the three CLI files, unit summary,
    triplex count and digest, Q1 and 148-250 counts."""
    man = helpers.read_manifest(os.path.join(golden_dir, f"peaks_{query}.manifest.gz"))
    assert len(peaks) == 532 and [r["idx"] for r in man] == list(range(532))
    assert [(r["header"], r["length"]) for r in man] == [(h, len(s)) for h, s in peaks]
    assert all(set(s) <= set(b"ACGT") for _, s in peaks)
    scans, files = _peak_detail(golden_dir, query)
    assert len(scans) >= 12 and sorted({i for i, _ in files}) == sorted(scans)
    for i, scan in scans.items():
        r = man[i]
        where = f"record {i} ({r['header']})"
        for kind in helpers.PEAK_FILES:
            assert helpers.file_digest(files[(i, kind)]) == (r[kind + "_lines"], r[kind + "_sha"]), (where, kind)
        meta, units = helpers.parse_scan(scan)
        assert meta["nseg"] == 1 and [u["enc"] for u in units] == list(range(48)), where
        summary = [(u["enc"], u["stage1"], u["thr"], u["colhash"], u["ncand"]) for u in units]
        assert helpers.unit_summary_digest(summary) == r["units"], where
        trips = helpers.expected_triplexes(units)
        assert (len(trips), helpers.triplex_digest(trips)) == (r["triplexes"], r["triplex_sha"]), where
        assert sum(u["stage1"] >= 251 for u in units) == r["q1"], where
        assert sum(148 <= u["stage1"] <= 250 for u in units) == r["rev148"], where
    # the selection holds the extremes it is meant to cover
    for key in ("triplexes", "q1", "length"):
        assert max(r[key] for r in man) == max(man[i][key] for i in scans), key
    assert min(r["length"] for r in man) == min(man[i]["length"] for i in scans)


@pytest.mark.parametrize("query", ["H19", "MALAT1"])
def test_peaks_fixture_covers_overflow_and_q2(golden_dir, query):
    """With H19 and MALAT1, real DNA drives units through byte overflow (Q1), the exact-reverse range and the signed
    lazy-F exit (Q2); a regenerated fixture must keep doing so."""
    man = helpers.read_manifest(os.path.join(golden_dir, f"peaks_{query}.manifest.gz"))
    assert sum(r["q1"] for r in man) > 0
    assert sum(r["rev148"] for r in man) > 0
    assert sum(r["q2"] for r in man) > 0


@pytest.mark.parametrize("query", helpers.PEAK_QUERIES)
def test_oracle_on_selected_peaks(oracle_build, golden_dir, peaks, tmp_path, query):
    """The oracle's scan and its three CLI files equal the reference's, byte for byte, for every selected peak record."""
    rna = os.path.join(golden_dir, query + ".fa")
    scans, files = _peak_detail(golden_dir, query)
    for i, scan in scans.items():
        hdr, seq = peaks[i]
        where = f"record {i} ({hdr})"
        dna = str(tmp_path / f"pk{i}.fa")
        synth.write_fasta(dna, hdr, seq)
        assert helpers.oracle_cli(oracle_build, "scan", rna, dna, "-detail", "0", "-threads", "8") == scan, where
        assert helpers.oracle_cli(oracle_build, "tfosorted", rna, dna, "-threads", "8") == files[(i, "TFOsorted")], where
        for level in (1, 2):
            out = helpers.oracle_cli(oracle_build, "tfoclass", rna, dna, "-level", str(level), "-threads", "8")
            assert out == files[(i, f"TFOclass{level}")], (where, level)


# ---- untidy queries: U, lower case, N and IUPAC letters in the lncRNA (`make_golden.py dirtyq`) ---------------------------------
def dirty_conditions(orc, rna, dna, units):
    """What the inputs of helpers.dirty_case must hold, from the oracle: the triplexes over each class of untidy row, the units
    whose stage-1 maximum exceeds every stage-2 column maximum (the two alphabets disagree about the threshold) as (segment,
    encoding, candidates), and the hazard (Q2) units that matter."""
    rows = helpers.dirty_rows(rna)
    xs = [x for u in units for x in u["triplexes"]]
    over = {k: sum(helpers.triplex_rows_overlap(x, r) for x in xs) for k, r in rows.items()}
    disagree = []
    for u in units:
        t, _ = orc.encode_unit(dna[u["seg"] * 4900:u["seg"] * 4900 + 5000], u["enc"])
        assert len(t) == u["n"]
        assert orc.stage1_max(rna, t) == u["stage1"]
        if u["stage1"] > max(orc.pre_align(rna, t)):
            disagree.append((u["seg"], u["enc"], u["ncand"]))
    return over, disagree, helpers.q2_units_that_matter(orc, rna, dna) if len(rna) >= 1300 else []


@pytest.mark.parametrize("m", helpers.DIRTY_LENGTHS)
def test_dirty_query_scan_and_input_conditions(oracle_build, golden_dir, tmp_path, m):
    """The oracle equals the reference on queries with a T-to-U stretch, a lower-case stretch and scattered N R Y n u (stage 1 reads U
    as T and the rest as N = -1; stages 2 and 3 read U as A and the rest as -4), and the generated inputs do what they are for:
    at least 5 expected triplexes over a U row, 5 over a lower-case row and 5 over an N / IUPAC row (the 100-nt query must hold the
    U and the lower-case class; its last third is 34 rows with one or two untidy letters), at least 3 units whose stage-1 maximum
    exceeds every stage-2 column maximum, one of them with a candidate, and for 1 300 and 4 000 rows a hazard unit."""
    rna_fa, dna_fa, rna, dna = helpers.dirty_case_files(tmp_path, m)
    zones = helpers.dirty_rows(rna)
    assert all(zones.values()) and set(rna) - set(b"ACGT") >= set(b"Uacgt") and set(rna) & set(b"NRYnu")
    assert set(dna) <= set(b"ACGT")
    gold = helpers.gunzip(os.path.join(golden_dir, f"dirtyq_{m}.scan.gz"))
    assert helpers.oracle_cli(oracle_build, "scan", rna_fa, dna_fa, "-detail", "0", "-threads", "8") == gold
    meta, units = helpers.parse_scan(gold)
    assert meta["m"] == m and meta["nseg"] == 3 and len(units) == 144 and not meta["skipped"]
    over, disagree, q2 = dirty_conditions(helpers.Oracle(oracle_build), rna, dna, units)
    print(f"m {m}: triplexes over untidy rows {over}, units with stage 1 above stage 2 {len(disagree)} ({sum(c > 0 for _, _, c in disagree)} with candidates), Q2 units {q2}")
    for kind in ("U", "lower") if m == 100 else ("U", "lower", "N"):
        assert over[kind] >= 5, (kind, over)
    assert len(disagree) >= 3 and any(c > 0 for _, _, c in disagree)
    if m >= 1300:
        assert len(q2) == helpers.DIRTY_Q2_UNITS[m] >= 1
        out = helpers.oracle_cli(oracle_build, "tfosorted", rna_fa, dna_fa, "-lg", "30", "-threads", "8")
        assert out == open(os.path.join(golden_dir, f"dirtyq_{m}.TFOsorted"), "rb").read()
        for level in (1, 2):
            out = helpers.oracle_cli(oracle_build, "tfoclass", rna_fa, dna_fa, "-lg", "30", "-level", str(level), "-threads", "8")
            assert out == open(os.path.join(golden_dir, f"dirtyq_{m}.TFOclass{level}"), "rb").read()


def test_dirty_query_probe_vectors(oracle_build, golden_dir):
    """S, P and A answers of the reference probe for a 900-nt untidy query against 40 targets and windows (every fourth with N and
    lower-case letters of its own): Oracle.stage1_max, pre_align and align."""
    o = helpers.Oracle(oracle_build)
    q, targets, wins, reqs = helpers.probe_dirty_vectors()
    rsp = helpers.gunzip(os.path.join(golden_dir, "probe_dirty40.rsp.gz")).decode().splitlines()
    assert len(rsp) == len(reqs) == 120
    assert any(set(t) & set(b"Nn") for t in targets) and any(set(t) & set(b"acgt") for t in targets)
    above, aligned = 0, 0
    for k in range(40):
        s1 = o.stage1_max(q, targets[k])
        cols = o.pre_align(q, targets[k])
        assert s1 == int(rsp[3 * k].split(" ")[1]), k
        assert cols == [int(x) for x in rsp[3 * k + 1].split(" ")[2:]], k
        above += s1 > max(cols)
        g = rsp[3 * k + 2].split(" ")
        five, cig = o.align(q, wins[k])
        if int(g[1]) == 0:
            assert five[0] == 0, k
        else:
            assert five == tuple(int(x) for x in g[1:6]) and (cig or "*") == g[6], k
            aligned += 1
    assert above >= 10 and aligned >= 30       # the alphabets disagree in many targets, and the windows do align
