"""Region scans: BED intervals of a genome FASTA (`fasim --regions`, Engine.scan_regions).  Each interval's files are those of
`fasim --all-records` for the record >NAME|CHROM|START+1-END that holds exactly the interval's bytes, which the reference's own
per-peak outputs pin down.  GPU only."""
import os
import random
import subprocess

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

SEVEN = ("segments", "segments_skipped", "units", "candidates", "align_calls", "logical_cells", "cells_stage2")
EXE = os.path.join(entry.PKG_DIR, "fasim")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def peaks(golden_dir):
    return helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))


def _rna(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))


def _run(wd, *args, env=None, check=True):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def _index(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "line\tname\tchrom\tstart\tend\tsegments\ttriplexes\tstem"
    return [dict(zip(lines[0].split("\t"), x.split("\t"))) for x in lines[1:]]


# ---- 1. the reference's 532 peaks as intervals of a "genome" of flanked records -----------------------------------------------
def test_peaks_genome_against_reference(golden_dir, peaks, tmp_path):
    """Every peak wrapped in 300 nt of synthetic flank under a reference-form header >hg19|chr|start-300-end+300; the BED lists the
    peaks' own intervals and names.  The 532 x 3 files equal the reference's files of each peak alone (record matching,
    coordinates and naming together), and the index counts each -TFOsorted's data lines."""
    fa, bed = [], []
    for k, (hdr, seq) in enumerate(peaks):
        name, chro, span = hdr.split("|")
        a, b = (int(x) for x in span.split("-"))
        flank = synth.random_dna(600, 7000 + k)
        fa.append(f">hg19|{chro}|{a - 300}-{b + 300}\n".encode() + flank[:300] + seq + flank[300:] + b"\n")
        bed.append(f"{chro}\t{a - 1}\t{b}\t{name}\n")
    (tmp_path / "peaks.fa").write_bytes(b"".join(fa))
    (tmp_path / "peaks.bed").write_text("track name=meg3_peaks\n" + "".join(bed))
    (tmp_path / "H19.fa").write_bytes(open(os.path.join(golden_dir, "H19.fa"), "rb").read())
    (tmp_path / "out").mkdir()
    _run(tmp_path, "-f1", "peaks.fa", "-f2", "H19.fa", "-O", "out/", "--regions", "peaks.bed")
    man = helpers.read_manifest(os.path.join(golden_dir, "peaks_H19.manifest.gz"))
    rna_name = _rna(golden_dir, "H19")[0]
    names = {}
    for r in man:
        species, chro = r["header"].split("|")[:2]
        stem = f"{species}-{rna_name}-peaks.{chro}"
        names[f"{stem}-TFOsorted"] = (r, "TFOsorted")
        for level in (1, 2):
            names[f"{stem}-TFOclass{level}-15-50"] = (r, f"TFOclass{level}")
    index = f"{rna_name}-peaks.regions.tsv"
    assert sorted(os.listdir(tmp_path / "out")) == sorted(list(names) + [index])
    bad = [f"record {r['idx']} ({r['header']}) {kind}" for name, (r, kind) in names.items()
           if helpers.file_digest((tmp_path / "out" / name).read_bytes()) != (r[kind + "_lines"], r[kind + "_sha"])]
    assert not bad, bad
    rows = _index(tmp_path / "out" / index)
    assert len(rows) == len(man)
    for row, r in zip(rows, man):
        species, chro = r["header"].split("|")[:2]
        assert (row["name"], row["chrom"], row["line"]) == (species, chro, str(r["idx"] + 2))
        assert row["stem"] == f"{species}-{rna_name}-peaks.{chro}" and row["segments"] == "1"
        assert int(row["triplexes"]) == r["TFOsorted_lines"] - 1


# ---- 2. a UCSC-style genome: edge intervals against --all-records on the extracted records ------------------------------------
def _ucsc_genome(peaks):
    """chrA and chrB from real DNA (the peaks joined), with headers as UCSC / Ensembl write them."""
    chra = b"".join(s for _, s in peaks[:10])
    chrb = b"".join(s for _, s in peaks[10:15])
    return {"chrA": chra, "chrB": chrb}


def _edge_bed(g):
    la, lb = len(g["chrA"]), len(g["chrB"])
    lines = [
        f"chrA\t100\t101\tone_nt",
        f"chrA\t1000\t5900\tlen4900",
        f"chrA\t2000\t6901\tlen4901",
        f"chrA\t3000\t8000",                          # 5 000 nt, generated name
        f"chrA\t{la - 3000}\t{la}\tchrA_tail",        # the last bases of a chromosome
        f"chrB\t{lb - 1}\t{lb}",                      # the very last base
        f"chrA\t10000\t16000\touter",
        f"chrA\t11000\t12500\tinner",                 # nested
        f"chrA\t15000\t19000\toverlap",               # overlaps `outer`
        f"chrA\t10000\t16000\touter",                 # identical line: the stem gets _<line>
        f"chrA\t10000\t16000\tsame_span",             # identical span, another name
        f"chrA\t500\t2500\tdup",
        f"chrB\t500\t2500\tdup",                      # same name, other chromosome
        f"chrA\t600\t2600\tdup",                      # same name and chromosome
        f"chrB\t0\t4000\tchrB_head",
    ]
    random.Random(5).shuffle(lines)                   # unordered lines
    return "".join(x + "\n" for x in lines)


def _write_genome(path, g):
    with open(path, "wb") as f:
        f.write(b">chrA\n" + g["chrA"] + b"\n")
        f.write(b">chrB AC:CM000664.2 gi|568336022|gb|CM000664.2| Homo sapiens chromosome B\n")   # '|' only after a space
        for k in range(0, len(g["chrB"]), 60):
            f.write(g["chrB"][k:k + 60] + b"\n")


def _extract(mod, bed_path, g):
    regs = mod.read_bed(bed_path)
    text = b"".join(f">{r.name}|{r.chrom}|{r.start + 1}-{r.end}\n".encode() + g[r.chrom][r.start:r.end] + b"\n" for r in regs)
    return regs, text


@pytest.fixture(scope="module")
def ucsc(mod, golden_dir, peaks, tmp_path_factory):
    """The --regions run on the UCSC-style genome and the --all-records run on the extracted records, with two lncRNAs."""
    base = tmp_path_factory.mktemp("ucsc")
    g = _ucsc_genome(peaks)
    rnas = b"".join(open(os.path.join(golden_dir, q + ".fa"), "rb").read() for q in ("H19", "MEG3"))
    for d in ("reg", "all"):
        (base / d / "out").mkdir(parents=True)
        (base / d / "q.fa").write_bytes(rnas)
    _write_genome(base / "reg" / "g.fa", g)
    (base / "reg" / "r.bed").write_text(_edge_bed(g))
    regs, text = _extract(mod, str(base / "reg" / "r.bed"), g)
    (base / "all" / "g.fa").write_bytes(text)
    _run(base / "all", "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", "--all-records")
    _run(base / "reg", "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", "--regions", "r.bed")
    return base, g, regs, [_rna(golden_dir, q)[0] for q in ("H19", "MEG3")]


def test_ucsc_genome_matches_all_records(ucsc):
    base, g, regs, lncs = ucsc
    got, want = _files(base / "reg" / "out"), _files(base / "all" / "out")
    index = {f"{n}-g.regions.tsv" for n in lncs}
    assert set(got) == set(want) | index
    assert len(want) == 3 * 2 * len(regs)
    assert [n for n in want if got[n] != want[n]] == []
    assert sum(b.count(b"\n") - 1 for n, b in want.items() if n.endswith("-TFOsorted")) > 0


def test_ucsc_index_counts_tfosorted_lines(mod, ucsc):
    base, g, regs, lncs = ucsc
    p = mod.default_params()
    for lnc in lncs:
        rows = _index(base / "reg" / "out" / f"{lnc}-g.regions.tsv")
        assert [(int(x["line"]), x["name"], x["chrom"], int(x["start"]), int(x["end"])) for x in rows] == \
            [(r.line, r.name, r.chrom, r.start, r.end) for r in regs]
        for x, r in zip(rows, regs):
            assert x["stem"] == f"{r.name}-{lnc}-g.{r.chrom}"
            data = (base / "reg" / "out" / (x["stem"] + "-TFOsorted")).read_bytes()
            assert int(x["triplexes"]) == data.count(b"\n") - 1
            assert int(x["segments"]) == mod.segment_count(r.end - r.start, p)


@pytest.mark.parametrize("how", ["devices_0_0", "no_groups"])
def test_ucsc_devices_and_ungrouped_give_the_same_files(ucsc, how):
    base, g, regs, _ = ucsc
    wd = base / "reg"
    out = wd / ("out_" + how)
    out.mkdir()
    if how == "devices_0_0":
        _run(wd, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--regions", "r.bed", "--devices", "0,0")
    else:
        _run(wd, "-f1", "g.fa", "-f2", "q.fa", "-O", out.name + "/", "--regions", "r.bed", env={"FASIM_RECORD_GROUP": "0"})
    assert _files(out) == _files(wd / "out")


def test_stats_line_per_interval(ucsc):
    base, g, regs, _ = ucsc
    wd = base / "reg"
    (wd / "out_stats").mkdir()
    r = _run(wd, "-f1", "g.fa", "-f2", "q.fa", "-O", "out_stats/", "--regions", "r.bed", "--stats")
    assert sum(1 for x in r.stderr.splitlines() if x.startswith("[fasim] record ")) == 2 * len(regs)


# ---- 3. unmatched intervals ----------------------------------------------------------------------------------------------------
def test_unmatched_intervals(mod, golden_dir, peaks, tmp_path):
    g = _ucsc_genome(peaks)
    _write_genome(tmp_path / "g.fa", g)
    lb = len(g["chrB"])
    (tmp_path / "q.fa").write_bytes(open(os.path.join(golden_dir, "H19.fa"), "rb").read())
    (tmp_path / "r.bed").write_text(f"chrA\t100\t900\tgood1\nchrZ\t0\t500\tnowhere\nchrB\t{lb - 50}\t{lb + 50}\tpast_end\n"
                                    f"chrB\t200\t800\tgood2\n")
    (tmp_path / "out").mkdir()
    r = _run(tmp_path, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", "--regions", "r.bed", check=False)
    assert r.returncode == 1, r.stderr
    assert "line 2 (nowhere) chrZ:0-500" in r.stderr and f"line 3 (past_end) chrB:{lb - 50}-{lb + 50}" in r.stderr, r.stderr
    assert "good1" not in r.stderr and "good2" not in r.stderr
    written = sorted(os.listdir(tmp_path / "out"))
    stems = ["good1-H19-g.chrA", "good2-H19-g.chrB"]
    assert written == sorted([s + x for s in stems for x in ("-TFOsorted", "-TFOclass1-15-50", "-TFOclass2-15-50")]
                             + ["H19-g.regions.tsv"])
    rows = _index(tmp_path / "out" / "H19-g.regions.tsv")
    assert [(x["name"], x["segments"], x["triplexes"], x["stem"]) for x in rows if x["segments"] == "NA"] == \
        [("nowhere", "NA", "NA", "NA"), ("past_end", "NA", "NA", "NA")]
    assert [x["stem"] for x in rows if x["segments"] != "NA"] == stems


# ---- 4. Engine.scan_regions: overlapping, nested, repeated, unordered spans ------------------------------------------------------
def _same(a, b):
    return a.triplexes() == b.triplexes() and a.recs == b.recs and a.pool == b.pool


SPANS = [(5000, 9000), (0, 2300), (5500, 6000), (5000, 9000), (8000, 12500), (100, 101), (2299, 7300), (20000, 23000), (0, 2300)]


@pytest.mark.parametrize("where", ["host", "resident"])
def test_scan_regions_equals_scan_records_of_slices(mod, golden_dir, peaks, where):
    seq = b"".join(s for _, s in peaks[:10])
    assert len(seq) > 23000
    p = mod.default_params(cLength=20)
    e = mod.Engine(0)
    try:
        e.set_query(_rna(golden_dir, "H19")[1])
        if where == "resident":
            e.load_dna(seq)
        res = e.scan_regions(seq if where == "host" else None, SPANS, p)
        tot = e.last_totals[0]
        want = e.scan_records([seq[s:t] for s, t in SPANS], p)
        assert len(res) == len(SPANS)
        for k, (x, y) in enumerate(zip(res, want)):
            assert _same(x, y), (k, SPANS[k])
            assert [x.stats[f] for f in SEVEN] == [y.stats[f] for f in SEVEN], (k, SPANS[k])
        assert tot["units"] == sum(x.stats["units"] for x in res)
        assert sum(x.count for x in res) > 0
        # several lncRNAs: the scan_queries shape
        rnas = [_rna(golden_dir, q)[1] for q in ("H19", "MEG3")]
        res2 = e.scan_regions(seq if where == "host" else None, SPANS[::-1], p, rnas=rnas)
        want2 = e.scan_records([seq[s:t] for s, t in SPANS[::-1]], p, rnas=rnas)
        for q in range(2):
            for k in range(len(SPANS)):
                assert _same(res2[q][k], want2[q][k]), (q, k)
        with pytest.raises(mod.FasimError):
            e.scan_regions(seq if where == "host" else None, [(10, 10)], p)
    finally:
        e.close()


# ---- 5. -F ----------------------------------------------------------------------------------------------------------------------
def test_classic_sim_regions(mod, golden_dir, tmp_path):
    """-F on three short intervals of the demo DNA (a reference-form record: chr11 from 2 158 478) equals --all-records -F on the
    extracted records."""
    hdr, demo = synth.read_fasta(os.path.join(golden_dir, "testDNA.fa"))
    _, chro, start = mod.parse_dna_header(hdr)
    g0 = start - 1
    spans = [(g0 + 1000, g0 + 1400), (g0 + 200, g0 + 700), (g0 + 3900, g0 + len(demo))]
    for d in ("reg", "all"):
        (tmp_path / d / "out").mkdir(parents=True)
        (tmp_path / d / "H19.fa").write_bytes(open(os.path.join(golden_dir, "H19.fa"), "rb").read())
    (tmp_path / "reg" / "demo.fa").write_bytes(open(os.path.join(golden_dir, "testDNA.fa"), "rb").read())
    (tmp_path / "reg" / "r.bed").write_text("".join(f"{chro}\t{s}\t{t}\n" for s, t in spans))
    (tmp_path / "all" / "demo.fa").write_bytes(b"".join(f">{chro}_{s + 1}_{t}|{chro}|{s + 1}-{t}\n".encode() + demo[s - g0:t - g0] + b"\n"
                                                        for s, t in spans))
    _run(tmp_path / "all", "-f1", "demo.fa", "-f2", "H19.fa", "-O", "out/", "-lg", "40", "-F", "--all-records")
    _run(tmp_path / "reg", "-f1", "demo.fa", "-f2", "H19.fa", "-O", "out/", "-lg", "40", "-F", "--regions", "r.bed")
    got, want = _files(tmp_path / "reg" / "out"), _files(tmp_path / "all" / "out")
    assert set(got) == set(want) | {"H19-demo.regions.tsv"} and len(want) == 9
    assert [n for n in want if got[n] != want[n]] == []
