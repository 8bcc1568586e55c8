"""The packed-f16 DP kernels (option dp_f16 / FASIM_DP_F16, csrc/dp_f16.h): the instruction they rest on, identical records
with the switch on and off, and the integer re-run of units whose scores leave the exact f16 range.  GPU only."""
import os

import numpy as np
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


def _rna(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _f16_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16).astype(np.uint32)


def test_maximum3_is_the_integer_maximum(mod):
    """For packed pairs of integer-valued f16 in [-4096, 4096] (every integer up to 2048, the even ones above), +0 and equal
    operands included, v_pk_maximum3_f16 must return the integer maximum bit for bit, with three registers and with the
    inline constant 0 as third operand.  All ordered triples of 128 values in the low half, other triples in the high half."""
    rng = np.random.default_rng(7)
    vals = np.array([0, 1, -1, 2, -2, 3, 5, -5, 8, -8, 10, -10, 31, 32, 33, 263, 264, -263, 511, 512, 1000, 1023, 1024, 1025,
                     2046, 2047, 2048, 2050, 2052, 3000, 4094, 4096, -1023, -1024, -2047, -2048, -2050, -4094, -4096], dtype=np.int64)
    extra = rng.integers(-4096, 4097, size=128 - len(vals))
    extra = np.where(np.abs(extra) > 2048, extra & ~1, extra)
    vals = np.concatenate([vals, extra])
    assert np.array_equal(vals.astype(np.float16).astype(np.int64), vals), "the operands must be exact in f16"
    nv = len(vals)
    i = np.arange(nv ** 3)
    lo = [vals[i % nv], vals[(i // nv) % nv], vals[i // (nv * nv)]]
    j = (i * 2654435761 + 12345) % (nv ** 3)
    hi = [vals[j // (nv * nv)], vals[j % nv], vals[(j // nv) % nv]]
    a, b, c = (_f16_bits(lo[k]) | (_f16_bits(hi[k]) << 16) for k in range(3))
    e = mod.Engine(0)
    out3, out0 = e.maximum3_f16(a, b, c)
    e.close()
    want3 = _f16_bits(np.maximum(np.maximum(lo[0], lo[1]), lo[2])) | (_f16_bits(np.maximum(np.maximum(hi[0], hi[1]), hi[2])) << 16)
    want0 = _f16_bits(np.maximum(np.maximum(lo[0], lo[1]), 0)) | (_f16_bits(np.maximum(np.maximum(hi[0], hi[1]), 0)) << 16)
    bad3, bad0 = np.flatnonzero(out3 != want3), np.flatnonzero(out0 != want0)
    assert bad3.size == 0, (bad3.size, [(hex(a[k]), hex(b[k]), hex(c[k]), hex(out3[k]), hex(want3[k])) for k in bad3[:4]])
    assert bad0.size == 0, (bad0.size, [(hex(a[k]), hex(b[k]), hex(out0[k]), hex(want0[k])) for k in bad0[:4]])


def _scan(mod, rna, dna, p, dp_f16):
    e = mod.Engine(0)
    e.set_option("dp_f16", dp_f16)
    e.set_query(rna)
    r = e.scan(dna, p)
    e.close()
    return r


def _joined_peaks(golden_dir):
    return b"".join(s for _, s in helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz")))


@pytest.mark.parametrize("query,dna_file", [("H19", "q2cat.fa"), ("H19", "planted40k.fa"), ("MALAT1", "malat1_dna.fa"),
                                            ("NEAT1", "neat1_dna.fa"), ("H19", "meg3_peaks")])
def test_dp_f16_switch_gives_identical_records(mod, golden_dir, query, dna_file):
    """dp_f16 = 0 (the integer kernels) and 1 (k_scan's main pass and the reverse pass of stage 3 in packed f16) give the same
    records and string pools: one query tile with Q2 hazard units (q2cat) and planted triplexes, 3 tiles (MALAT1), 8 tiles
    (NEAT1) and the 532 real ChIP peak sequences as one record."""
    rna = _rna(golden_dir, query)
    dna = _joined_peaks(golden_dir) if dna_file == "meg3_peaks" else synth.read_fasta(os.path.join(golden_dir, dna_file))[1]
    p = mod.default_params(cLength=20)
    r0, r1 = _scan(mod, rna, dna, p, 0), _scan(mod, rna, dna, p, 1)
    assert r0.count > 0 and r0.stats["kernel_launches"][0] > 0 and r1.stats["kernel_launches"][0] > 0
    assert r0.stats["dp_f16_reruns"] == 0
    print(f"{query} x {dna_file}: {r1.stats['units']} units, {r1.stats['dp_f16_reruns']} re-run on the integer kernel, "
          f"{r1.stats['rev_bound_passes']} reverse passes, {r1.stats['hazard_units']} hazard units")
    assert (r1.recs, r1.pool) == (r0.recs, r0.pool)
    for k in ("candidates", "align_calls", "hazard_units", "band_tries", "band_proven", "rev_bound_passes", "stage2_overflow_units"):
        assert r1.stats[k] == r0.stats[k], k


def test_unit_beyond_the_exact_range_is_rerun(mod, golden_dir, oracle_build):
    """A segment that holds the exact pre-image of 260 nt of H19 under a one-to-one rule encoding scores about 1 300 there, beyond
    the 1 023 the f16 k_scan holds exactly.  The oracle (CPU) says which of the 48 units reach 1 024; exactly those must be
    handed to the integer kernel, and the records must be those of dp_f16 = 0."""
    rna = _rna(golden_dir, "H19")
    enc = 26
    out = synth.RULE_OUT[enc]                       # outputs for the DNA letters A, T, G, C
    assert len(set(out)) == 4 and not synth.enc_reversed(enc)
    pre = {o: base for base, o in zip("ATGC", out)}
    window = rna[700:960].decode().upper().replace("U", "T")
    assert set(window) <= set("ACGT")
    dna = bytearray(synth.random_dna(3000, 4242))
    dna[1200:1200 + len(window)] = "".join(pre[ch] for ch in window).encode()
    dna = bytes(dna)
    orc = helpers.Oracle(oracle_build)
    scores = [orc.stage1_max(rna, orc.encode_unit(dna, k)[0]) for k in range(48)]
    beyond = [k for k in range(48) if scores[k] >= 1024]
    print("stage-1 maxima >= 1024:", {k: scores[k] for k in beyond})
    assert enc in beyond and scores[enc] >= 1024
    p = mod.default_params(cLength=20)
    r0, r1 = _scan(mod, rna, dna, p, 0), _scan(mod, rna, dna, p, 1)
    assert r0.stats["units"] == 48 and r0.stats["dp_f16_reruns"] == 0
    assert r1.stats["dp_f16_reruns"] > 0
    assert r1.stats["dp_f16_reruns"] == len(beyond)
    assert r0.count > 0 and (r1.recs, r1.pool) == (r0.recs, r0.pool)
    assert r1.stats["candidates"] == r0.stats["candidates"] and r1.stats["hazard_units"] == r0.stats["hazard_units"]


def _edited_preimage(rows: str, enc: int, edits: str):
    """The exact pre-image of `rows` under a one-to-one encoding with one edit every 25 bases, at offsets 25, 50, 75, ...:
    x another base (a mismatch), i a second base behind it (an insertion), d the base left out (a deletion)."""
    out = synth.RULE_OUT[enc]
    assert len(set(out)) == 4 and not synth.enc_reversed(enc)
    pre = {o: base for base, o in zip("ATGC", out)}
    assert set(rows) <= set(pre)
    tract = [pre[ch] for ch in rows]
    for n, op in enumerate(edits):
        k = 25 * (n + 1)
        other = "ACGT"[("ACGT".index(tract[k]) + 1) % 4]
        tract[k] = {"x": other, "i": tract[k] + other, "d": ""}[op]
    return "".join(tract).encode()


# (query, first planted row, planted rows, edits).  With H19 the oracle scores the unit of encoding 26 at 1 022, 1 023, 1 024, 1 025
# and 1 031: both sides of the last exactly held score, 1 023, and the lumps next to them.  The last two are queries of the
# rows-per-lane sweep: RP 17, and RP 2, the smallest build whose query (256 rows, 1 280 at the most) can leave the range at all
# (RP 1 is at most 128 rows, 640).
F16_EDGE_CASES = (("H19", 700, 200, ""), ("H19", 700, 208, "ii"), ("H19", 700, 210, "xii"), ("H19", 700, 204, "d"), ("H19", 700, 201, ""),
                  (2176, 1000, 260, "x"), (256, 0, 256, ""))


def test_ends_of_the_exact_range(mod, golden_dir, oracle_build):
    """Carried values are 2 * score + taint, exact up to 2 047, and the flag fires at a block maximum of 2 048: a unit that scores
    1 023 is NOT run again and its f16 results stand, a unit that scores 1 024 is.  For every case the oracle gives the stage-1
    maximum of all 48 units; exactly the units at 1 024 or more are re-run, and records and pool are those of the integer kernels.
    The cases hold a unit in [1016, 1023] and one in [1024, 1031] (asserted here, from the oracle)."""
    orc = helpers.Oracle(oracle_build)
    enc = 26
    p = mod.default_params(cLength=20)
    below, above, rps = [], [], set()
    for query, row0, nrows, edits in F16_EDGE_CASES:
        rna = _rna(golden_dir, query) if isinstance(query, str) else helpers.row_layout_inputs(query)[0]
        rows = rna[row0:row0 + nrows].decode().upper().replace("U", "T")
        assert len(rows) == nrows
        tract = _edited_preimage(rows, enc, edits)
        dna = bytearray(synth.random_dna(3000, 4242))
        dna[1200:1200 + len(tract)] = tract
        dna = bytes(dna)
        scores = [orc.stage1_max(rna, orc.encode_unit(dna, k)[0]) for k in range(48)]
        beyond = [k for k in range(48) if scores[k] >= 1024]
        rp = helpers.systolic_layout(len(rna))[2]
        print(f"{query} rows [{row0}, {row0 + nrows}) edits '{edits}': RP {rp}, encoding {enc} scores {scores[enc]}, "
              f"units >= 1024: {({k: scores[k] for k in beyond})}")
        below += [s for s in scores if 1016 <= s <= 1023]
        above += [s for s in scores if 1024 <= s <= 1031]
        if beyond:
            rps.add(rp)
        r0, r1 = _scan(mod, rna, dna, p, 0), _scan(mod, rna, dna, p, 1)
        assert r0.stats["units"] == 48 and r0.stats["dp_f16_reruns"] == 0
        assert r1.stats["dp_f16_reruns"] == len(beyond), (query, nrows, edits)
        assert r0.count > 0 and (r1.recs, r1.pool) == (r0.recs, r0.pool), (query, nrows, edits)
        assert r1.stats["candidates"] == r0.stats["candidates"]
    assert below and above, (below, above)
    print("scores in [1016, 1023]:", sorted(below), "in [1024, 1031]:", sorted(above))
    assert min(rps) <= 2 and max(rps) >= 17 and 22 in rps, rps
