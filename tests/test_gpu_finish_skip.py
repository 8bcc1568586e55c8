"""Option finish_skip / FASIM_FINISH_SKIP (align.hip k_finish_rev / k_finish_trace, csrc/doomed.h): by default the
scan's finish leaves an alignment without its CIGAR when the stability filter is certain to drop its record; 0 traces every
alignment on k_finish_lds as before; 2 traces everything and checks the rule against the full conversion
(stats finish_skip_violations).  The three settings must give the same records and string pools, byte for byte, and the
reference's records where a fixture holds them.  GPU only.

cLength is set equal to ntMin, so that LongTarget's tail filter equals fastSIM's."""
import os

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

TIERS = ("finish_lds16", "finish_lds64", "finish_glob16k", "finish_glob1m")
ENC, ENC_REV = 22, 23            # one-to-one encodings of rule 6, antiparallel: 22 reads forwards and shows the complement, 23 reads backwards


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def h19(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]


def scan(mod, rna, dna, mode, p=None):
    e = mod.Engine(0)
    e.set_option("finish_skip", mode)
    e.set_query(rna)
    r = e.scan(dna, p or mod.default_params(cLength=20))
    out = {"trips": r.triplexes(), "recs": r.recs, "pool": r.pool, "stats": dict(r.stats)}
    del r
    e.close()
    return out


def finished(st):
    return sum(st[k] for k in TIERS)


def three_modes(mod, rna, dna, what, p=None):
    """scans with finish_skip 0, 1 and 2: the same records and pools, no violation, and mode 2 marks what mode 1 leaves out"""
    got = [scan(mod, rna, dna, v, p) for v in (0, 1, 2)]
    st = [g["stats"] for g in got]
    print(f"{what}: {len(got[0]['trips'])} triplexes, finished {finished(st[1])}, skipped {st[1]['finish_skipped']}, "
          f"violations {st[2]['finish_skip_violations']}, finish family ms {st[0]['kernel_ms'][3]:.3f} / {st[1]['kernel_ms'][3]:.3f}")
    for v in (1, 2):
        assert got[v]["recs"] == got[0]["recs"] and got[v]["pool"] == got[0]["pool"], (what, v)
        assert st[v]["candidates"] == st[0]["candidates"] and st[v]["align_calls"] == st[0]["align_calls"], (what, v)
    assert st[0]["finish_skipped"] == 0 and st[0]["finish_skip_violations"] == 0 and st[1]["finish_skip_violations"] == 0
    assert st[2]["finish_skip_violations"] == 0, what
    assert st[2]["finish_skipped"] == st[1]["finish_skipped"], what
    assert finished(st[1]) == finished(st[0]) == finished(st[2]), what
    return got[1]


# ---- (a) plain input ------------------------------------------------------------------------------------------------------------
def test_random_dna_three_modes(mod, h19):
    """H19 x 60 kb of random DNA.  On the CPU, 67 % of the reference's finished alignments of such input hold a TT pair and are long
    enough (counted after the de-duplication, a floor): at least half must be skipped, so the test cannot pass empty."""
    got = three_modes(mod, h19, synth.random_dna(60_000, 12345), "random 60 kb")
    st = got["stats"]
    assert finished(st) > 1000 and 2 * st["finish_skipped"] >= finished(st), (st["finish_skipped"], finished(st))


# ---- (b) fixtures at the default parameters -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dna_file,fixture", [("testDNA.fa", "demo.scan.gz"), ("planted40k.fa", "planted40k.scan.gz")])
def test_default_fixtures(mod, h19, golden_dir, dna_file, fixture):
    _, dna = synth.read_fasta(os.path.join(golden_dir, dna_file))
    _, units = helpers.parse_scan(helpers.gunzip(os.path.join(golden_dir, fixture)))
    got = scan(mod, h19, dna, 1)
    assert got["trips"] == helpers.expected_triplexes(units)
    assert got["stats"]["finish_skipped"] > 0 and got["stats"]["finish_skip_violations"] == 0
    if dna_file == "planted40k.fa":
        # (f) its long plants score 148 and more: their begin comes from the exact reverse pass, and they are never left out
        assert got["stats"]["rev_exact"] > 0 and got["stats"]["finish_skipped"] < finished(got["stats"])


# ---- (c) other parameters: the rule adapts or switches off ----------------------------------------------------------------------
# pen: -S -50, nothing fails the filter.  pen_stab / pen_stab_swapped: penaltyT -3 / -2 with -S 1: 4.5 (nt - 1) - 3 < nt - 1 only for
# nt = 1, which holds no pair.  thresholds (-S 2) and ntmax (-na 40: longer alignments have stability 0) keep the default penalty.
@pytest.mark.parametrize("name,skips", [("pen", False), ("pen_stab", False), ("pen_stab_swapped", False), ("thresholds", True), ("ntmax", True)])
def test_parameter_sets(mod, golden_dir, name, skips):
    query, dna_file, options = helpers.SCAN_PARAM_PINNED[name]
    _, dna = helpers.scan_param_dna(golden_dir, name, dna_file)
    _, units = helpers.scan_param_fixture(golden_dir, name)
    fields = helpers.scan_option_fields(options)
    p = mod.default_params(**fields)
    if "cLength" not in fields:
        p.cLength = p.ntMin
    rna = synth.read_fasta(os.path.join(golden_dir, query + ".fa"))[1]
    got = [scan(mod, rna, dna, v, p) for v in (1, 2)]
    for g in got:
        assert g["trips"] == helpers.expected_triplexes(units), name
    assert got[0]["recs"] == got[1]["recs"] and got[0]["pool"] == got[1]["pool"]
    assert got[1]["stats"]["finish_skip_violations"] == 0
    assert (got[0]["stats"]["finish_skipped"] > 0) == skips, (name, got[0]["stats"]["finish_skipped"])
    assert got[1]["stats"]["finish_skipped"] == got[0]["stats"]["finish_skipped"]


# ---- (d) letters that complement() drops ----------------------------------------------------------------------------------------
def test_unclean_segments_keep_their_strand_1_units(mod, h19):
    """-t 1 (the parallel rules: encodings 0 .. 11, every second one shows the complement).  One IUPAC letter or N per segment makes
    every segment unclean: the units that show the complement are then never skipped, the others are."""
    clean = bytearray(synth.random_dna(3 * 4900 + 100, 777))
    dirty = bytearray(clean)
    for pos, ch in ((50, b"R"), (2500, b"N"), (4950, b"Y"), (7000, b"n"), (9850, b"K"), (12000, b"N")):      # 4950, 9850: in two segments each
        dirty[pos:pos + 1] = ch
    p = mod.default_params(cLength=20, strand=1)
    got_clean = three_modes(mod, h19, bytes(clean), "clean, -t 1", p)
    got_dirty = three_modes(mod, h19, bytes(dirty), "N and IUPAC, -t 1", p)
    a, b = got_clean["stats"]["finish_skipped"], got_dirty["stats"]["finish_skipped"]
    assert a > 100 and 0 < b < 0.75 * a, (a, b)      # about half: six letters change few of the alignments themselves


# ---- (e), (f) a record that is one alignment, from its first to its last column ----------------------------------------------------
def _plant(rna, length, enc, want_pair):
    """the exact pre-image of `length` query rows under encoding enc, read from the record's first to its last column; the first
    rows for which the shown strand holds a TT pair (under encoding 22, which shows the complement, the DNA an AA pair) -- or none"""
    shows_complement = (enc & 1) if enc < 12 else 1 - ((enc - 12) & 1)
    pair = b"AA" if shows_complement else b"TT"
    for r0 in range(100, len(rna) - length, 7):
        tract = helpers.preimage(rna[r0:r0 + length], enc, synth._Rng(r0))
        if tract is not None and (pair in bytes(tract)) == want_pair:
            return bytes(tract)              # (in DNA order already: the odd encoding reads it from its last letter)
    raise AssertionError("no such rows")


@pytest.mark.parametrize("enc", [ENC, ENC_REV])
@pytest.mark.parametrize("length", [24, 29])
def test_alignment_over_the_whole_segment(mod, h19, enc, length):
    """The span of the unit's alignment is [0, n - 1] (mirrored index n - 1 ... 0 under the odd encoding): the TT test reads the
    segment's first and last letter and nothing beyond.  Scores 120 and 145: below 148."""
    dna = _plant(h19, length, enc, True)
    p = mod.default_params(cLength=20, rule=6, strand=-1)
    got = three_modes(mod, h19, dna, f"plant of {length} rows, enc {enc}", p)
    assert got["stats"]["units"] == 2 and got["stats"]["finish_skipped"] >= 1, got["stats"]
    three_modes(mod, h19, _plant(h19, length, enc, False), f"plant of {length} rows without a pair, enc {enc}", p)


@pytest.mark.parametrize("enc", [ENC, ENC_REV])
def test_scores_from_148_are_never_skipped(mod, h19, enc):
    """35 rows, score 175: the begin comes from the exact reverse pass, and the alignment keeps its CIGAR although its span holds a
    pair."""
    dna = _plant(h19, 35, enc, True)
    p = mod.default_params(cLength=20, rule=6, strand=-1)
    got = three_modes(mod, h19, dna, f"plant of 35 rows, enc {enc}", p)
    st = got["stats"]
    assert st["rev_exact"] >= 1 and st["finish_skipped"] < finished(st), st
