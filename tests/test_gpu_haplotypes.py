"""Variants scored on a sample's phased haplotypes, on the GPU (fasim_score_haplotypes, k_hap_encode, `fasim --variants --sample`).
A haplotype score is, by definition, fasim_score_variants on the record that carries the haplotype's other variants: every test
compares values, encodings and clip bit with the numpy restatement of section 19 (test_variants_cpu.expected_scores) on the records
that test_haplotypes_cpu.edited_record edits with byte strings, and with the existing Engine.score_variants on those same edited
records.  GPU only."""
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_gpu_oligos import _pre_image
from test_haplotypes_cpu import _other, edited_record, expected_info, hap_windows, HEAD
from test_track_cpu import enabled_encodings, encode_unit
from test_variants_cpu import expected_scores

pytestmark = pytest.mark.gpu

EXE = os.path.join(entry.PKG_DIR, "fasim")
LDS_PIECES = 64          # HAP_LDS_PIECES (csrc/kernels.h): piece ends of a window that k_hap_encode searches in LDS


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    return mod.Engine(0)


def _query(golden_dir, m: int) -> bytes:
    return synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1][200:200 + m]


def edited_problems(mod, dna, variants, gts, matched, flank, only=None):
    """The definition's own problems: (records, variants on them, slot[v, h]) -- one edited record and one variant at a' per distinct
    pair of windows (of the entries `only`, or of all)."""
    recs, evars, index = [], [], {}
    slot = np.full((len(variants), 2), -1, dtype=np.int64)
    for v, x in enumerate(variants):
        if not x.usable or (only is not None and v not in only):
            continue
        for h in range(2):
            r, a, _ = edited_record(dna, variants, gts, matched, v, h)
            key = hap_windows(dna, variants, gts, matched, v, h, flank)[0]
            if key not in index:
                index[key] = len(evars)
                recs.append(r)
                evars.append(mod.Variant(x.line, x.chrom, a, x.id, x.ref, x.alt, len(recs) - 1))
            slot[v, h] = index[key]
    return recs, evars, slot


def check(mod, eng, query, dna, variants, gts, flank, p, what, matched=None, restate=True):
    """score_haplotypes against the restatement (restate) and against score_variants, both on the edited records; the planner's part
    of info against test_haplotypes_cpu.expected_info.  Returns (values, encs, info) of the query."""
    values, encs, info = eng.score_haplotypes(variants, gts, [dna], p, flank=flank, queries=[query], matched=matched)
    assert values.shape == (1, len(variants), 2, 2, 4) and encs.shape == values.shape and info.shape == (1, len(variants), 2, 3)
    values, encs, info = values[0], encs[0], info[0]
    recs, evars, slot = edited_problems(mod, dna, variants, gts, matched, flank)
    plain = [x[0] for x in eng.score_variants(evars, recs, p, flank=flank, queries=[query])]
    both = [(plain, "score_variants on the edited records")]
    if restate:
        both.append((expected_scores(query, recs, evars, flank, p), "restatement"))
    for exp, name in both:
        for v, x in enumerate(variants):
            for h in range(2):
                if not x.usable:
                    assert values[v, h].max() == 0 and encs[v, h].max() == -1 and info[v, h, 1:].tolist() == [0, 0]
                    continue
                k = slot[v, h]
                assert values[v, h].tolist() == np.asarray(exp[0][k]).tolist(), (what, name, "values", v, h)
                assert encs[v, h].tolist() == np.asarray(exp[1][k]).tolist(), (what, name, "encs", v, h)
                assert info[v, h, 2] & 1 == int(exp[2][k]), (what, name, "clip bit", v, h)
    for v, x in enumerate(variants):
        if x.usable:
            exp = expected_info(dna, variants, gts, matched, v, flank)
            assert info[v, :, :2].tolist() == exp[:, :2].tolist() and (info[v, :, 2] & ~1).tolist() == exp[:, 2].tolist(), (what, v)
    return values, encs, info


# ---- 1. nothing applies ------------------------------------------------------------------------------------------------------------
def _simple(mod, seed=3, n=3000):
    dna = bytearray(synth.random_dna(n, seed))
    dna[1480:1540] = b"AGGAGAAGGAGAGGAAGAGAGGAAGGAGAAGGGAGAGAGGAAGAGGAGAAGGAGAGGAGA"
    dna = bytes(dna)
    V = mod.Variant
    at = (0, 700, 1500, 1510, 1520, 2200, n - 1)
    variants = [V(k + 1, "c", a, f"s{k}", dna[a:a + 1].decode(), _other(dna[a:a + 1])) for k, a in enumerate(at)]
    variants.insert(3, V(20, "c", 1505, "ins", dna[1505:1506].decode(), dna[1505:1506].decode() + "GA"))
    variants.insert(4, V(21, "c", 1600, "sym", dna[1600:1601].decode(), "<DEL>", 0, False))
    return dna, variants


@pytest.mark.parametrize("gt", [(0, 0, 1), (0, 1, 0), (-1, -1, 0), (0, 0, 0)], ids=["0|0", "0/1", "missing", "0/0"])
def test_nothing_applies_equals_score_variants(mod, eng, golden_dir, gt):
    p = mod.default_params()
    query = _query(golden_dir, 100)
    dna, variants = _simple(mod)
    gts = np.array([gt] * len(variants), dtype=np.int8)
    values, encs, info = eng.score_haplotypes(variants, gts, [dna], p, flank=300, queries=[query])
    pv, pe, pf = eng.score_variants(variants, [dna], p, flank=300, queries=[query])
    assert pv.max() > 0
    for h in range(2):
        assert np.array_equal(values[:, :, h], pv) and np.array_equal(encs[:, :, h], pe)
        assert np.array_equal(info[0, :, h, 2] & 1, pf[0])
    usable = np.array([v.usable for v in variants])
    assert (info[0, usable, :, 2] & 8).all() and (info[0, :, :, 1] == 0).all()
    assert (info[0, :, :, 0] == np.array(gt[:2])).all()
    # a far neighbour changes nothing either: an entry 400 bases away with a flank of 300
    gts[1] = (1, 1, 1)
    again = eng.score_haplotypes(variants, gts, [dna], p, flank=300, queries=[query])
    assert np.array_equal(again[0], values) and np.array_equal(again[1], encs)


# ---- 2. clustered entries -----------------------------------------------------------------------------------------------------------
def clustered_record(mod, query, p, n_entries, seed, length=8000, centres=(1500, 3500, 5500, 7000)):
    """An 8 kb record: a purine tract, pre-images of a stretch of the query under the first forward and the first reversed enabled
    encoding at the clusters' centres, and n_entries entries in clusters (steps of 1 to 12 bases) with random phased genotypes."""
    rng = np.random.default_rng(seed)
    dna = bytearray(synth.random_dna(length, seed))
    dna[centres[1] - 100:centres[1] + 100] = bytes(b"AG"[int(c)] for c in rng.integers(0, 2, 200))
    encs = enabled_encodings(p)
    for at, enc in zip(centres[:1] + centres[2:], (encs[0], next(e for e in encs if e & 1), encs[-1])):
        pre = _pre_image(query[:min(len(query), 60)], enc, rng)
        dna[at - len(pre) // 2:at - len(pre) // 2 + len(pre)] = pre
    dna = bytes(dna)
    variants, gts = [], []
    per = (n_entries + len(centres) - 1) // len(centres)
    for c in centres:
        at = c - 4 * per
        for _ in range(min(per, n_entries - len(variants))):
            at += int(rng.integers(1, 13))
            kind = int(rng.integers(0, 10))
            nref = int(rng.integers(2, 9)) if kind == 7 else 3 if kind == 8 else 1
            ref = dna[at:at + nref].decode()
            alt = ref[0] if kind == 7 else ref + "".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(1, 9)))) if kind == 9 \
                else _other(dna[at:at + nref])
            variants.append(mod.Variant(len(variants) + 1, "c", at, f"e{len(variants)}", ref, alt))
            gts.append(((1, 0, 1), (0, 1, 1), (1, 1, 1), (0, 0, 1), (1, 0, 1), (0, 1, 1))[int(rng.integers(0, 6))])
    return dna, variants, np.array(gts, dtype=np.int8)


@pytest.mark.parametrize("flank", [0, 30, 300])
@pytest.mark.parametrize("m", [20, 100, 150])
def test_clustered_entries_equal_the_edited_records(mod, eng, golden_dir, m, flank):
    """Workgroups of 64, 128 and 256 threads; all 48 encodings; about 60 entries, most with several neighbours in reach, some
    overlapping (rejected), insertions and deletions among them.  The numpy restatement walks 120 edited records x 48 encodings x 2
    alleles column by column: 23 s and 38 s for the 100- and the 150-nt query at flank 300, so there the yardstick is score_variants on
    the edited records alone (itself held to the restatement by test_gpu_variants.py); the 20-nt query has both at every flank."""
    p = mod.default_params()
    assert len(enabled_encodings(p)) == 48
    query = _query(golden_dir, m)
    dna, variants, gts = clustered_record(mod, query, p, 60, 17)
    values, encs, info = check(mod, eng, query, dna, variants, gts, flank, p, f"m={m} flank={flank}", restate=m * flank <= 6000)
    assert values.max() > 0
    if flank:
        assert (info[:, :, 1] > 1).sum() > 30 and (info[:, :, 2] & 4).any() and not (info[:, :, 2] & 8).all()
        assert (values[:, 0] != values[:, 1]).any()


def test_widest_flank_with_six_entries(mod, eng, golden_dir):
    p = mod.default_params()
    query = _query(golden_dir, 20)
    dna, variants, gts = clustered_record(mod, query, p, 6, 23, centres=(1500, 3500))
    gts[:, :] = [(1, 0, 1), (1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
    values, _, info = check(mod, eng, query, dna, variants, gts, 2048, p, "flank=2048")
    assert values.max() > 0 and (info[:, :, 1] > 0).all()


# ---- 3. the two-mismatch 30-mer -----------------------------------------------------------------------------------------------------
def test_two_mismatches_on_one_haplotype(mod, eng):
    """A planted 30-mer with two mismatches five bases apart, both repaired by ALT on haplotype 0.  Scored against the reference each
    variant is 132 -> 141; the carrier's change is 141 -> 150 on that haplotype and nothing on the other."""
    q = b"TGGTTGTGGTGTTGGTGGTTGTGTGGTTGT"
    pre = q.replace(b"T", b"a").replace(b"G", b"T").replace(b"a", b"A")
    assert encode_unit(pre, 0) == q
    swap = {65: 84, 84: 65}
    bad = bytearray(pre)
    for col in (11, 16):
        bad[col] = swap[bad[col]]
    dna = b"N" * 50 + bytes(bad) + b"N" * 50
    variants = [mod.Variant(k + 1, "c", 50 + col, f"m{col}", chr(bad[col]), chr(pre[col])) for k, col in enumerate((11, 16))]
    gts = np.array([(1, 0, 1), (1, 0, 1)], dtype=np.int8)
    p = mod.default_params(rule=1, strand=1)
    pv, pe, pf = eng.score_variants(variants, [dna], p, flank=40, queries=[q])
    assert pv[0, :, :, 0].tolist() == [[132, 141], [132, 141]]                       # plain deltas: 9 and 9
    values, encs, info = check(mod, eng, q, dna, variants, gts, 40, p, "two mismatches")
    assert values[:, 0, :, 0].tolist() == [[141, 150], [141, 150]]                  # max_ref, max_alt on the carrying haplotype
    assert np.array_equal(values[:, 1], pv[0]) and np.array_equal(encs[:, 1], pe[0])      # the other one: the plain score
    assert info[:, :, 0].tolist() == [[1, 0], [1, 0]] and info[:, :, 1].tolist() == [[1, 0], [1, 0]]
    assert not (info[:, :, 2] & 8).any()


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------
def test_order_residence_and_queries_do_not_matter(mod, golden_dir):
    e = mod.Engine(0)
    p = mod.default_params(rule=1)
    queries = [_query(golden_dir, 40), _query(golden_dir, 130)]
    dna, variants, gts = clustered_record(mod, queries[1], p, 30, 29)
    base = e.score_haplotypes(variants, gts, [dna], p, flank=100, queries=queries)
    assert base[0].max() > 0 and (base[2][..., 1] > 0).any()
    perm = np.random.default_rng(1).permutation(len(variants))
    got = e.score_haplotypes([variants[k] for k in perm], gts[perm], [dna], p, flank=100, queries=queries)
    for a, b in zip(base, got):
        assert np.array_equal(a[:, perm], b)
    for q, query in enumerate(queries):
        one = e.score_haplotypes(variants, gts, [dna], p, flank=100, queries=[query])
        for a, b in zip(base, one):
            assert np.array_equal(a[q], b[0])
    e.load_dna(dna)
    resident = e.score_haplotypes(variants, gts, None, p, flank=100, queries=queries)
    for a, b in zip(base, resident):
        assert np.array_equal(a, b)
    # and two records in one call: the second one's entries see their own record only
    dna2 = synth.random_dna(500, 31)
    more = variants + [mod.Variant(900, "d", 250, "r1", dna2[250:251].decode(), _other(dna2[250:251]), 1),
                       mod.Variant(901, "d", 255, "r1b", dna2[255:256].decode(), _other(dna2[255:256]), 1)]
    gts2 = np.concatenate([gts, np.array([(1, 1, 1), (1, 0, 1)], dtype=np.int8)])
    both = e.score_haplotypes(more, gts2, [dna, dna2], p, flank=100, queries=queries)
    for a, b in zip(base, both):
        assert np.array_equal(a, b[:, :len(variants)])
    assert both[2][0, -2:, :, 1].tolist() == [[1, 0], [1, 1]]


# ---- 5. more pieces than the LDS stage holds ------------------------------------------------------------------------------------------
def test_a_window_with_more_pieces_than_the_lds_stage(mod, eng, golden_dir):
    """201 adjacent SNVs on haplotype 0 and every other one on haplotype 1: windows of up to 301 pieces (haplotype 0: every letter a
    piece of its own) and of about 150, so that k_hap_encode searches most letters in HBM; forward and reversed encodings."""
    p = mod.default_params(rule=1)
    query = _query(golden_dir, 20)
    dna = bytearray(synth.random_dna(1000, 9))
    pre = _pre_image(query, enabled_encodings(p)[0], np.random.default_rng(2))
    dna[490:490 + len(pre)] = pre
    dna = bytes(dna)
    variants = [mod.Variant(k + 1, "c", 400 + k, f"a{k}", dna[400 + k:401 + k].decode(), _other(dna[400 + k:401 + k])) for k in range(201)]
    gts = np.array([(1, k & 1, 1) for k in range(201)], dtype=np.int8)
    focus = [0, 1, 60, 100, 101, 199, 200]      # (every entry is scored, seven are compared: the restatement stays small)
    values, encs, info = eng.score_haplotypes(variants, gts, [dna], p, flank=150, queries=[query])
    recs, evars, slot = edited_problems(mod, dna, variants, gts, None, 150, only=focus)
    pick = sorted({int(slot[v, h]) for v in focus for h in range(2)})
    sub = [evars[k]._replace(rec=i) for i, k in enumerate(pick)]
    want = expected_scores(query, [recs[evars[k].rec] for k in pick], sub, 150, p)
    plain = [x[0] for x in eng.score_variants(sub, [recs[evars[k].rec] for k in pick], p, flank=150, queries=[query])]
    assert info[0, 100, 0, 1] == 200 > LDS_PIECES and info[0, 100, 1, 1] == 100 > LDS_PIECES
    for exp in (want, plain):
        for v in focus:
            for h in range(2):
                k = pick.index(int(slot[v, h]))
                assert values[0, v, h].tolist() == np.asarray(exp[0][k]).tolist(), (v, h)
                assert encs[0, v, h].tolist() == np.asarray(exp[1][k]).tolist(), (v, h)
                assert info[0, v, h, 2] & 1 == int(exp[2][k])
    assert values[0, focus].max() > 0


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_table_equals_the_python_results(mod, eng, tmp_path, golden_dir):
    q = _query(golden_dir, 60)
    p = mod.default_params()
    dna, variants, gts = clustered_record(mod, q, p, 12, 37, length=6000, centres=(1500, 3500, 5000))
    synth.write_fasta(str(tmp_path / "g.fa"), "chr1 test record", dna)
    (tmp_path / "q.fa").write_text(">Q\n" + q.decode() + "\n")
    fmt = {(1, 0, 1): "1|0", (0, 1, 1): "0|1", (1, 1, 1): "1|1", (0, 0, 1): "0|0"}
    lines = [HEAD]
    for k, (v, g) in enumerate(zip(variants, gts)):
        ref = _other(v.ref.encode()) if k == 5 else v.ref                             # one entry whose REF differs from the record
        lines.append(f"chr1\t{v.pos + 1}\t{v.id}\t{ref}\t{v.alt}\t.\t.\t.\tDP:GT\t9:0/1\t7:{fmt[tuple(int(x) for x in g)]}\n")
    lines.insert(4, "chr1\t1\tstar\t" + dna[:1].decode() + "\t*\t.\t.\t.\tGT\t0|1\t1|1\n")
    (tmp_path / "v.vcf").write_text("".join(lines))
    outs = {}
    for name, extra in (("plain", ()), ("hap", ("--sample", "S2"))):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([EXE, "-f1", "g.fa", "-f2", "q.fa", "-O", name + "/", "--variants", "v.vcf", "--variant-flank", "150", *extra],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "2 of 13 variants were not scored" in r.stderr, r.stderr
        outs[name] = {f: (out / f).read_bytes() for f in os.listdir(out)}
    assert sorted(outs["plain"]) == ["Q-g.variants.tsv"] and sorted(outs["hap"]) == ["Q-g.haplotypes.tsv", "Q-g.variants.tsv"]
    assert outs["hap"]["Q-g.variants.tsv"] == outs["plain"]["Q-g.variants.tsv"]
    entries, genotypes = mod.read_vcf(str(tmp_path / "v.vcf"), sample="S2")
    assert len(entries) == 13
    matched = [v.usable and v.ref.encode() == dna[v.pos:v.pos + len(v.ref)] for v in entries]
    assert matched.count(False) == 2
    values, encs, info = eng.score_haplotypes(entries, genotypes, [dna], p, flank=150, queries=[q], matched=matched)
    want = mod.haplotypes_tsv(entries, genotypes, values[0], encs[0], info[0], 150, "Q", "S2", matched=matched)
    assert outs["hap"]["Q-g.haplotypes.tsv"] == want
    assert (info[0, :, :, 1] > 0).any() and want.count(b"\tNA" * 35 + b"\n") == 2
