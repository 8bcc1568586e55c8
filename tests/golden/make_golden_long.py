#!/usr/bin/env python3
"""Regenerate the long-query fixtures of tests/golden/ from the compiled reference (oracle/_ref, built by `make -C oracle ref`).

Only runs where the reference binaries exist.  Everything written here is DATA: inputs and the reference's outputs for them.

  longq92k.fa      92 256 nt (FASIM_MAX_QUERY): NEAT1 + MALAT1 + MEG3 + H19, the 4 000-nt satq.fa block, then
                   synth.random_rna(.., 9256) up to the exact length
  longq49k.fa      its first 49 153 nt (the shortest query past 16 systolic tiles)
  longq_dna.fa     one 25 kb DNA record: synth.planted_dna(20000, 9256, longq92k, every=600) with a lower-case letter every
                   997 nt and one N run, then a 5 kb block with unmutated 3 950 ... 3 990-nt copies of the satq part
                   (the stage-1 score of such a unit leaves the 8-bit range at once)
  longq92k.scan.gz / longq49k.scan.gz          ref_probe `scan -detail 0`
  longq92k_lg40.TFO* / longq49k_lg40.TFO*      the reference CLI's three output files with -lg 40

The set is checked for what the long-query tests need: units whose stage-1 score saturates the 16-bit k_scan lanes
(>= 16 383), candidates and triplexes for both queries.  The four reference runs go side by side (about 1.5 minutes).
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
FASIM = os.path.join(ROOT, "oracle", "_ref", "fasim_ref")
MAX_QUERY = 92256
SHORT = 49153


def long_query():
    parts = [synth.read_fasta(os.path.join(GOLD, n + ".fa"))[1] for n in ("NEAT1", "MALAT1", "MEG3", "H19")]
    satq = synth.read_fasta(os.path.join(GOLD, "satq.fa"))[1]
    q = b"".join(parts) + satq
    assert len(q) < SHORT, "the satq block must lie within the first 49 153 nt"
    q += synth.random_rna(MAX_QUERY - len(q), 9256)
    assert len(q) == MAX_QUERY
    return q, satq


def long_dna(q, satq):
    d = bytearray(synth.planted_dna(20000, 9256, q, every=600))
    for pos in range(500, len(d), 997):
        d[pos] = d[pos] | 0x20                  # single lower-case letters
    d[7000:7400] = b"N" * 400
    sat = synth.planted_dna(5000, 1, satq, every=10, min_len=3950, max_len=3990, mut_pct=0, indel_pct=0)
    return bytes(d) + sat


def write_gz(path, data):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
        g.write(data)


def main():
    assert os.path.exists(PROBE) and os.path.exists(FASIM), "run `make -C oracle ref` first"
    q, satq = long_query()
    dna = long_dna(q, satq)
    hdr = f"syn|chrL|1-{len(dna)}"
    synth.write_fasta(os.path.join(GOLD, "longq92k.fa"), "LONGQ92K", q)
    synth.write_fasta(os.path.join(GOLD, "longq49k.fa"), "LONGQ49K", q[:SHORT])
    synth.write_fasta(os.path.join(GOLD, "longq_dna.fa"), hdr, dna)
    wd = tempfile.mkdtemp(prefix="fasim_gold_long_")
    try:
        for f in ("longq92k.fa", "longq49k.fa", "longq_dna.fa"):
            shutil.copyfile(os.path.join(GOLD, f), os.path.join(wd, f))
        procs = []
        for stem in ("longq92k", "longq49k"):
            out = os.path.join(wd, "out_" + stem)
            os.makedirs(out)
            procs.append((stem, "cli", out, subprocess.Popen([FASIM, "-f1", "longq_dna.fa", "-f2", stem + ".fa", "-O", out + "/", "-lg", "40"],
                                                               cwd=wd, stdout=subprocess.DEVNULL)))
            procs.append((stem, "scan", None, subprocess.Popen([PROBE, "scan", stem + ".fa", "longq_dna.fa", "-detail", "0"], cwd=wd,
                                                                stdout=subprocess.PIPE)))
        scans = {}
        for stem, kind, out, pr in procs:
            if kind == "scan":
                text, _ = pr.communicate()
                assert pr.returncode == 0, stem
                scans[stem] = text
                write_gz(os.path.join(GOLD, stem + ".scan.gz"), text)
            else:
                assert pr.wait() == 0, stem
                for f in os.listdir(out):
                    data = open(os.path.join(out, f), "rb").read()
                    if f.endswith("-TFOsorted"):
                        open(os.path.join(GOLD, stem + "_lg40.TFOsorted"), "wb").write(data)
                    elif "-TFOclass" in f:
                        level = int(f.split("-TFOclass")[1].split("-")[0])
                        open(os.path.join(GOLD, f"{stem}_lg40.TFOclass{level}"), "wb").write(data)
            print(stem, kind, "done", flush=True)
    finally:
        shutil.rmtree(wd, ignore_errors=True)

    # coverage of the set
    sat = 0
    for stem, text in scans.items():
        _, units = helpers.parse_scan(text)
        sat += sum(1 for u in units if u["stage1"] >= 16383)
        assert sum(u["ncand"] for u in units) > 0 and sum(len(u["triplexes"]) for u in units) > 0, stem
    assert sat > 0, "no unit saturates the 16-bit k_scan lanes"
    for f in ("longq92k.fa", "longq49k.fa", "longq_dna.fa", "longq92k.scan.gz", "longq49k.scan.gz"):
        assert os.path.getsize(os.path.join(GOLD, f)) < 1 << 20, f
    print(f"coverage: {sat} saturated units")


if __name__ == "__main__":
    main()
