"""Variants scored on a sample's phased haplotypes (fasim_score_haplotypes), the part that needs no GPU: the
reader of genotypes, the host planner against an independent restatement of the definition, the table, the CLI's usage errors.

The restatement never calls the code under test: it picks the consistent set of a haplotype by the definition's greedy rule, applies
the neighbours of a focus entry to the record with byte-string edits, and takes the windows of the edited record from
test_variants_cpu.windows -- a haplotype score is, by definition, fasim_score_variants on that edited record.  The GPU tests
(test_gpu_haplotypes.py) use the same functions for their expected scores."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_variants_cpu import BAD_VCF, CLASS_NAMES, windows

MAX_ALLELE = 1024


def _mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(autouse=True)
def _feature():
    m = _mod()
    assert "fasim_score_haplotypes" in m.EXPORTS and hasattr(m.lib(), "fasim_score_haplotypes")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _meet(a, b):
    return a.pos < b.pos + len(b.ref) and b.pos < a.pos + len(a.ref)


def _qualifies(variants, gts, matched, k, h):
    g = gts[k]
    return bool(variants[k].usable and (matched is None or matched[k]) and g[h] == 1 and (g[2] or (g[0] == 1 and g[1] == 1)))


def consistent_set(variants, gts, matched, h, rec):
    """A_h of record `rec`: entry indices in the order they were accepted."""
    order = sorted((k for k, v in enumerate(variants) if v.rec == rec), key=lambda k: (variants[k].pos, variants[k].line, k))
    acc = []
    for k in order:
        if _qualifies(variants, gts, matched, k, h) and not any(_meet(variants[k], variants[u]) for u in acc):
            acc.append(k)
    return acc


def applied_neighbours(variants, gts, matched, v, h):
    x = variants[v]
    return [u for u in consistent_set(variants, gts, matched, h, x.rec) if variants[u].line != x.line and not _meet(variants[u], x)]


def edited_record(dna: bytes, variants, gts, matched, v, h):
    """(R_h(v), a', [(entry, first letter of its ALT in R_h, ALT length)])"""
    x = variants[v]
    nb = applied_neighbours(variants, gts, matched, v, h)
    r = dna
    for u in sorted(nb, key=lambda u: -variants[u].pos):
        y = variants[u]
        assert r[y.pos:y.pos + len(y.ref)] == dna[y.pos:y.pos + len(y.ref)]
        r = r[:y.pos] + y.alt.encode() + r[y.pos + len(y.ref):]
    shift = 0
    at = []
    a = x.pos
    for u in sorted(nb, key=lambda u: variants[u].pos):
        y = variants[u]
        at.append((u, y.pos + shift, len(y.alt)))
        shift += len(y.alt) - len(y.ref)
        if y.pos < x.pos:
            a = x.pos + shift
    return r, a, at


def hap_windows(dna: bytes, variants, gts, matched, v, h, flank):
    """(ref window, alt window, v0, edge_lo, edge_hi) of entry v on haplotype h, and the applied neighbours with a letter in them."""
    x = variants[v]
    r, a, at = edited_record(dna, variants, gts, matched, v, h)
    w = windows(r, a, len(x.ref), x.alt.encode(), flank)
    lo, hi = max(0, a - flank), min(len(r), a + len(x.ref) + flank)
    return w, sum(1 for _, p, n in at if p < hi and lo < p + n)


def expected_info(dna: bytes, variants, gts, matched, v, flank):
    """(2, 3): carried, applied, flags without the clip bit."""
    x = variants[v]
    out = np.zeros((2, 3), dtype=np.int64)
    win = []
    for h in range(2):
        g = gts[v]
        others = [u for u, y in enumerate(variants) if u != v and y.rec == x.rec and y.line == x.line and gts[u][h] == 1]
        out[h, 0] = 1 if g[h] == 1 else -1 if g[h] < 0 else 2 if others else 0
        w, out[h, 1] = hap_windows(dna, variants, gts, matched, v, h, flank)
        win.append(w)
        acc = set(consistent_set(variants, gts, matched, h, x.rec))
        for u, y in enumerate(variants):
            if y.rec != x.rec or y.line == x.line or abs(y.pos - x.pos) > flank + MAX_ALLELE:
                continue
            if y.usable and (matched is None or matched[u]) and gts[u][h] == 1 and not gts[u][2] and not (gts[u][0] == 1 and gts[u][1] == 1):
                out[h, 2] |= 2
            if _qualifies(variants, gts, matched, u, h) and (u not in acc or _meet(y, x)):
                out[h, 2] |= 4
    if win[0] == win[1]:
        out[:, 2] |= 8
    return out


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
def _vcf(tmp_path, text, name="v.vcf"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"


def test_read_vcf_sample_genotypes(tmp_path):
    m = _mod()
    text = (HEAD +
            "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|1\t1|0\n"
            "chr1\t20\tb\tA\tG\t.\t.\t.\tGT:DP\t1|0:7\t1/1:3\n"
            "chr1\t30\tc\tA\tG\t.\t.\t.\tGT\t1/1\t0/1\n"
            "chr1\t40\td\tA\tG\t.\t.\t.\tGT\t0/1\t./.\n"
            "chr1\t50\te\tA\tG\t.\t.\t.\tGT\t./.\t1\n"
            "chr1\t60\tf\tA\tG\t.\t.\t.\tGT\t1\t.\n"
            "chr1\t70\tg\tAC\tA,ACGT,<DEL>\t.\t.\t.\tGT\t1|2\t3|0\n"            # one entry per ALT: each asks for its own index
            "chr1\t80\th\tA\tG\t.\t.\t.\tDP:GQ:GT\t5:9:0|1\t5:9:.|1\r\n"          # GT not first in FORMAT; CRLF
            "chr1\t90\ti\tA\tG\t.\t.\t.\tGT\t0|0\t1|.\n")
    path = _vcf(tmp_path, text)
    plain = m.read_vcf(path)
    want = {"S1": [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (-1, -1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 1)],
            "S2": [(1, 0, 1), (1, 1, 0), (0, 1, 0), (-1, -1, 0), (1, 1, 1), (-1, -1, 1), (0, 0, 1), (0, 0, 1), (1, 0, 1), (-1, 1, 1), (1, -1, 1)]}
    for sample, exp in want.items():
        variants, gts = m.read_vcf(path, sample=sample)
        assert variants == plain                                     # the entries are fasim_read_vcf's
        assert gts.dtype == np.int8 and gts.shape == (len(plain), 3)
        assert [tuple(int(x) for x in g) for g in gts] == exp, sample
    assert [v.usable for v in plain[6:9]] == [True, True, False]
    v, g = m.read_vcf(_vcf(tmp_path, HEAD, "empty.vcf"), sample="S2")
    assert v == [] and g.shape == (0, 3)


BAD_SAMPLE = [
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|1\t1|0\n", "S3", 2, "names no sample 'S3'"),
    ("chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|1\t1|0\n", "S1", 1, "no #CHROM line"),
    ("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "chr1\t10\ta\tA\tG\n", "S1", 1, "names no sample 'S1'"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|1\t1|0\nchr1\t20\tb\tA\tG\t.\t.\t.\tGT\t0|1\n", "S2", 4, "no column of sample 'S2'"),
    (HEAD + "chr1\t20\tb\tA\tG\n", "S1", 3, "no column of sample 'S1'"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tDP:GQ\t5:9\t5:9\n", "S1", 3, "no GT in FORMAT"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|x\t1|0\n", "S1", 3, "malformed GT '0|x'"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|2\t1|0\n", "S1", 3, "malformed GT '0|2'"),          # the line has one ALT
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t0|1|1\t1|0\n", "S1", 3, "malformed GT '0|1|1'"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t|1\t1|0\n", "S1", 3, "malformed GT '|1'"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t\t1|0\n", "S1", 3, "malformed GT ''"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tDP:GT\t5\t5:1|0\n", "S1", 3, "malformed GT ''"),
    (HEAD + "chr1\t10\ta\tA\tG\t.\t.\t.\tGT\t-1|0\t1|0\n", "S1", 3, "malformed GT '-1|0'"),
]


@pytest.mark.parametrize("text,sample,line,reason", BAD_SAMPLE, ids=[f"{i}-{b[3].split()[0]}" for i, b in enumerate(BAD_SAMPLE)])
def test_read_vcf_sample_refusals_name_the_line_and_the_reason(tmp_path, text, sample, line, reason):
    m = _mod()
    with pytest.raises(m.FasimError) as ei:
        m.read_vcf(_vcf(tmp_path, text), sample=sample)
    assert ei.value.code == m.E_ARG
    assert f"line {line}:" in str(ei.value) and reason in str(ei.value), str(ei.value)


@pytest.mark.parametrize("text,line,reason", BAD_VCF, ids=[b[2].split()[0] + str(i) for i, b in enumerate(BAD_VCF)])
def test_read_vcf_sample_keeps_the_refusals_of_read_vcf(tmp_path, text, line, reason):
    m = _mod()
    # (every line of five columns gets the sample's columns, so that the first refusal is still the one of the case)
    text = "".join(x + ("\t.\t.\t.\tGT\t0|1\t0|1" if x.count("\t") == 4 else "") + "\n" for x in text.split("\n")[:-1])
    with pytest.raises(m.FasimError) as ei:
        m.read_vcf(_vcf(tmp_path, HEAD + text), sample="S1")
    assert ei.value.code == m.E_ARG
    assert f"line {line + 2}:" in str(ei.value) and reason in str(ei.value), str(ei.value)


# ---- the planner against the restatement --------------------------------------------------------------------------------------------
def _other(letters: bytes) -> str:
    return bytes({65: 67, 67: 71, 71: 84, 84: 65, 78: 65}[c] for c in letters).decode()


def clustered_case(m, length=3000, seed=5):
    """(record, variants, genotypes, matched): a 3 kb record with the constellations the definition has a word for (each laid out
    for a flank of 30) and a cluster of random entries, several within 50 bp."""
    dna = synth.random_dna(length, seed)
    rng = np.random.default_rng(seed)
    V = m.Variant
    rows = []

    def add(pos, nref, alt, gt, matched=True, usable=True, line=None):
        ref = dna[pos:pos + nref].decode()
        if alt == "snv":
            alt = _other(dna[pos:pos + nref])
        elif alt == "del":
            alt = ref[0]
        elif isinstance(alt, int):
            alt = ref + "".join("ACGT"[c] for c in rng.integers(0, 4, alt))
        rows.append((line if line is not None else len(rows) + 1, pos, ref, alt, gt, matched, usable))

    P0, P1, HOM, UH, UHOM, NONE, MISS = (1, 0, 1), (0, 1, 1), (1, 1, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1), (-1, -1, 0)
    add(0, 1, "snv", HOM); add(10, 1, "snv", P0)                                   # a neighbour at the record's first base
    add(510, 1, 5, P0); add(520, 8, "del", P0); add(540, 1, "snv", P0)             # an insertion and a deletion left of a focus
    add(700, 1, "snv", P1); add(725, 1, 19, P1)                                    # a neighbour's ALT cut by the window's end
    add(900, 1, "snv", P0); add(910, 1, 24, P0); add(925, 1, "snv", P0)            # inside 30 reference bases, outside 30 letters
    add(1100, 1, "snv", P1); add(1105, 20, "del", P1); add(1140, 1, "snv", P1)     # outside 30 reference bases, inside 30 letters
    add(1300, 10, "del", HOM); add(1305, 1, "snv", HOM); add(1320, 1, "snv", P0)   # two overlapping neighbours
    add(1500, 3, "snv", P1); add(1501, 1, "snv", HOM); add(1510, 1, "snv", HOM)    # a neighbour that overlaps the focus
    add(1700, 1, "snv", UH); add(1710, 1, "snv", UHOM); add(1720, 1, "snv", P0)    # unphased: a heterozygote, a homozygote
    add(1900, 1, "snv", HOM, matched=False); add(1910, 1, "snv", P1)               # an unmatched entry
    add(2100, 2, "snv", P0, line=90); add(2100, 2, 3, P1, line=90); add(2110, 1, "snv", HOM)      # 1|2 on one line
    add(2200, 1, "<DEL>", HOM, usable=False); add(2210, 1, "snv", NONE)
    add(2300, 1, "snv", MISS); add(2305, 1, "snv", (1, -1, 1))
    at = 2400
    for k in range(10):                                                            # the cluster
        at += int(rng.integers(1, 25))
        kind = int(rng.integers(0, 4))
        gt = (P0, P1, HOM, NONE, P0, P1)[int(rng.integers(0, 6))]
        add(at, (1, 1, int(rng.integers(2, 9)), 3)[kind], ("snv", int(rng.integers(1, 9)), "del", "snv")[kind], gt)
    add(2985, 1, "snv", P0); add(2995, 5, "del", P0); add(2999, 1, "snv", P1)      # neighbours at the record's last bases
    variants = [V(line, "c", pos, f"e{k}", ref, alt, 0, usable) for k, (line, pos, ref, alt, gt, mt, usable) in enumerate(rows)]
    gts = np.array([r[4] for r in rows], dtype=np.int8)
    matched = [r[5] for r in rows]
    return dna, variants, gts, matched


@pytest.mark.parametrize("flank", [0, 30, 300, 2048])
def test_planner_equals_the_restatement(flank):
    m = _mod()
    dna, variants, gts, matched = clustered_case(m)
    assert 38 <= len(variants) <= 45
    seen = np.zeros(4, dtype=np.int64)
    applied_total = 0
    for v, x in enumerate(variants):
        if not x.usable:
            with pytest.raises(m.FasimError):
                m.haplotype_window(variants, gts, dna, v, 0, 0, flank, matched=matched)
            continue
        info = expected_info(dna, variants, gts, matched, v, flank)
        got = m.haplotype_info(variants, gts, dna, v, flank, matched=matched)
        assert got.tolist() == info.tolist(), (flank, v, x)
        for b in range(4):
            seen[b] += int(((info[:, 2] >> b) & 1).any())
        applied_total += int(info[:, 1].sum())
        for h in range(2):
            (ref_w, alt_w, v0, e_lo, e_hi), _ = hap_windows(dna, variants, gts, matched, v, h, flank)
            for allele, w in enumerate((ref_w, alt_w)):
                letters, g0, edge = m.haplotype_window(variants, gts, dna, v, h, allele, flank, matched=matched)
                assert (letters, g0, edge) == (w, v0, int(e_lo) | int(e_hi) << 1), (flank, v, h, allele)
    # (bit 0 is the kernel's; with 2 048 letters on each side every window of this record holds a difference of the haplotypes)
    assert seen[0] == 0 and (seen[1:3] > 0).all() and (seen[3] > 0) == (flank < 2048), seen
    assert (applied_total > 0) == (flank > 0)
    if flank == 30:
        # the laid-out constellations are what they say
        def applied(v, h):
            return int(expected_info(dna, variants, gts, matched, v, 30)[h, 1])
        ids = {x.id: k for k, x in enumerate(variants)}
        assert applied(ids["e4"], 0) == 2 and applied(ids["e4"], 1) == 0            # the insertion and the deletion
        w, n = hap_windows(dna, variants, gts, matched, ids["e5"], 1, 30)
        assert n == 1 and w[0].endswith(variants[ids["e6"]].alt[:6].encode()) and w[4]      # the ALT is cut after six letters
        assert applied(ids["e7"], 0) == 1 and applied(ids["e10"], 1) == 2
        assert applied(ids["e15"], 0) == 1                                           # of the two overlapping, the first
        assert applied(ids["e21"], 0) == 1 and applied(ids["e21"], 1) == 1          # the unphased homozygote only
        assert applied(ids["e23"], 0) == 0 and applied(ids["e23"], 1) == 0          # the unmatched entry is never applied


def test_nothing_applied_gives_the_plain_windows():
    m = _mod()
    dna, variants, gts, matched = clustered_case(m)
    none = np.zeros_like(gts)
    none[:, 2] = 1
    for v, x in enumerate(variants):
        if not x.usable:
            continue
        want = windows(dna, x.pos, len(x.ref), x.alt.encode(), 300)
        for h in range(2):
            for allele in range(2):
                letters, v0, edge = m.haplotype_window(variants, none, dna, v, h, allele, 300)
                assert (letters, v0, edge) == (want[allele], want[2], int(want[3]) | int(want[4]) << 1)
        assert m.haplotype_info(variants, none, dna, v, 300).tolist() == [[0, 0, 8], [0, 0, 8]]


def test_a_run_of_adjacent_neighbours_is_walked_piece_by_piece():
    """100 adjacent SNVs on haplotype 0 left and right of a focus: 201 pieces and more in a window of flank 150."""
    m = _mod()
    dna = synth.random_dna(1000, 9)
    V = m.Variant
    variants = [V(k + 1, "c", 400 + k, ".", dna[400 + k:401 + k].decode(), _other(dna[400 + k:401 + k])) for k in range(201)]
    gts = np.array([(1, 0, 1)] * 201, dtype=np.int8)
    for v in (0, 100, 200):
        for h in range(2):
            (ref_w, alt_w, v0, e_lo, e_hi), n = hap_windows(dna, variants, gts, None, v, h, 150)
            assert n == (0 if h else min(v, 150) + min(200 - v, 150))
            assert m.haplotype_window(variants, gts, dna, v, h, 1, 150) == (alt_w, v0, int(e_lo) | int(e_hi) << 1)


# ---- fasim_haplotypes_tsv -----------------------------------------------------------------------------------------------------------
def tsv_head(name, sample, flank):
    cols = ["line", "chrom", "pos", "id", "ref", "alt", "gt"]
    for h in ("h1", "h2"):
        cols += [f"{h}_carried", f"{h}_applied"]
        for c in CLASS_NAMES:
            cols += [f"{h}_{c}_ref", f"{h}_{c}_alt"]
        cols += [f"{h}_{c}" for c in ("max_ref", "max_alt", "delta", "rule_ref", "rule_alt", "value", "flags")]
    return f"# fasim haplotypes lncRNA={name} sample={sample} flank={flank}\n" + "\t".join(cols + ["diplotype_max"]) + "\n"


def test_haplotypes_tsv_bytes():
    m = _mod()
    V = m.Variant
    variants = [V(3, "chr1", 99, "rs1", "A", "G"), V(4, "chr1", 199, ".", "AC", "A"), V(4, "chr1", 199, ".", "AC", "<DEL>", 0, False),
                V(7, "chr9", 0, "lost", "T", "C"), V(8, "chr1", 299, "flat", "T", "C")]
    gts = [(0, 1, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1), (-1, 1, 1)]
    values = np.zeros((5, 2, 2, 4), dtype=np.int32)
    encs = np.full((5, 2, 2, 4), -1, dtype=np.int32)
    info = np.zeros((5, 2, 3), dtype=np.int32)
    values[0, 0] = [[50, 0, 75, 75], [41, 0, 84, 60]]
    encs[0, 0] = [[2, -1, 16, 13], [2, -1, 18, 47]]          # rules: enc 16 -> 3, enc 18 -> 4
    values[0, 1] = [[0, 20, 0, 0], [0, 0, 0, 0]]
    encs[0, 1] = [[-1, 11, -1, -1], [-1, -1, -1, -1]]        # enc 11 -> rule 6
    info[0] = [[0, 0, 0], [1, 2, 5]]
    values[1] = values[0, 0]
    encs[1] = encs[0, 0]
    info[1] = [[1, 0, 8], [1, 0, 8]]
    values[3] = 999                                            # not matched: never printed
    info[4] = [[-1, 0, 0], [2, 1, 2]]
    got = m.haplotypes_tsv(variants, gts, values, encs, info, 300, "MEG3", "NA12878", matched=[1, 1, 1, 0, 1])
    na = "\tNA" * 35 + "\n"
    h_a = "\t50\t41\t0\t0\t75\t84\t75\t60\t75\t84\t9\t3\t4"
    want = (tsv_head("MEG3", "NA12878", 300) +
            "3\tchr1\t100\trs1\tA\tG\t0|1\t0\t0" + h_a + "\t75\t0" + "\t1\t2\t0\t0\t20\t0\t0\t0\t0\t0\t20\t0\t-20\t6\tNA\t0\t5" + "\t75\n"
            "4\tchr1\t200\t.\tAC\tA\t1/1\t1\t0" + h_a + "\t84\t8" + "\t1\t0" + h_a + "\t84\t8" + "\t84\n"
            "4\tchr1\t200\t.\tAC\t<DEL>\t0/0" + na +
            "7\tchr9\t1\tlost\tT\tC\t1|0" + na +
            "8\tchr1\t300\tflat\tT\tC\t.|1\t-1\t0" + "\t0" * 11 + "\tNA\tNA\tNA\t0" + "\t2\t1" + "\t0" * 11 + "\tNA\tNA\tNA\t2" + "\tNA\n")
    assert got == want.encode()
    assert m.haplotypes_tsv([], np.zeros((0, 3)), np.zeros((0, 2, 2, 4)), np.zeros((0, 2, 2, 4)), np.zeros((0, 2, 3)), 0, "q", "s") == \
        tsv_head("q", "s", 0).encode()


def test_haplotype_symbols_are_exported():
    m = _mod()
    for s in ("fasim_read_vcf_sample", "fasim_haplotype_window", "fasim_haplotype_info", "fasim_score_haplotypes", "fasim_haplotypes_tsv"):
        assert s in m.EXPORTS and hasattr(m.lib(), s)
    for name in ("haplotype_window", "haplotype_info", "haplotypes_tsv"):
        assert callable(getattr(m, name))
    assert callable(m.Engine.score_haplotypes)
    hdr = open(os.path.join(entry.ROOT, "include", "fasim_hip.h")).read()
    assert "typedef struct fasim_genotype { int8_t hap[2]; uint8_t phased, pad; } fasim_genotype;" in hdr
    assert "typedef struct fasim_hap_score { fasim_variant_score hap[2]; int32_t carried[2], applied[2], flags[2]; } fasim_hap_score;" in hdr


# ---- the CLI: usage errors and bad files exit 2 before any engine exists and write nothing --------------------------------------
def _cli(tmp_path, *args):
    _mod()
    exe = os.path.join(entry.PKG_DIR, "fasim")
    (tmp_path / "g.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "q.fa").write_text(">Q\n" + "AGAGGAAGAG" * 6 + "\n")
    if not (tmp_path / "v.vcf").exists():
        (tmp_path / "v.vcf").write_text(HEAD + "chr1\t10\trs1\tC\tG\t.\t.\t.\tGT\t0|1\t1|1\n")
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, "-f1", "g.fa", "-f2", "q.fa", "-O", "out/", *args], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    return r, sorted(os.listdir(out))


def test_cli_sample_needs_variants(tmp_path):
    r, written = _cli(tmp_path, "--sample", "S1")
    assert r.returncode == 2 and "--sample needs --variants" in r.stderr, r.stderr
    assert written == []


@pytest.mark.parametrize("text,sample,line,reason", BAD_SAMPLE, ids=[f"{i}-{b[3].split()[0]}" for i, b in enumerate(BAD_SAMPLE)])
def test_cli_exits_2_on_the_readers_refusals(tmp_path, text, sample, line, reason):
    _vcf(tmp_path, text)
    r, written = _cli(tmp_path, "--variants", "v.vcf", "--sample", sample)
    assert r.returncode == 2, r.stderr
    assert f"line {line}:" in r.stderr and reason in r.stderr, r.stderr
    assert written == []


def test_cli_empty_sample_name_exits_2(tmp_path):
    r, written = _cli(tmp_path, "--variants", "v.vcf", "--sample", "")
    assert r.returncode == 2 and "--sample" in r.stderr, r.stderr
    assert written == []
