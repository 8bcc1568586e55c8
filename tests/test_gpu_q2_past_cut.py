"""Option q2_past_cut / FASIM_Q2_PAST_CUT (scan.hip): by default k_scan stops tracking Q2 taints 128 pipeline
steps after a block of 64 steps whose maximum is >= 251 and clean, because k_scan_post reads no taint behind the overflow cut that
such a value proves; with the option at 1 it tracks to the end of every unit.  Both settings must give the oracle's records, and
the same records, string pools and counters as each other.

How the inputs are built.  Every case but the last two is ONE segment of 5 000 columns, scanned with H19 (2 812 rows: stripes of 176
rows, 22 rows per virtual lane, so row r lives in virtual lane r // 22 and meets column c at pipeline step c + r // 22).
  * Background: a segment of tests/golden/q2cat.fa.  Its own Q2 sites score 150 ... 250; a unit that also holds an overflow has a
    threshold of at least 204 (0.8 x 255), under which most of them no longer matter.
  * The Q2 site: the gapped plant of helpers.ROW_LAYOUT_GAP_PLANTS at the LAST stripe boundary b = 15 x 176, rows [b - 48, b) and
    [b + 26, b + 47) back to back.  F enters row b at 224, the reference's signed lazy-F exit withholds the 124 that the second part
    starts from, and the textbook 124 + 105 = 229 is above 204.  The taints are set in virtual lanes 120 and 121, 120 steps after
    lane 0 has seen the column.
  * The overflow: the exact pre-image of query rows [0, 51) (synth.planted_dna's kind of plant, unmutated), 255 on one diagonal.
    Its first cell >= 251 is row 50, virtual lane 2, at column (first column of the plant) + 50.
  With the overflow right behind the Q2 site, lane 2 proves the cut, and the block of 64 steps closes, BEFORE lanes 120 / 121 set the
  taints of columns that lie before the cut (test_cut_is_proven_before_the_taints_are_set): a kernel that switched the tracking off
  when the block closes, and not 128 steps later, loses the unit's hazard flag, and with it the records (tried once with such a
  build: the cases at distance 1 fail, profiles/r22_q2_past_cut.txt section 9).
"Q2 matters" is the criterion of test_gpu_parity._q2_units_that_matter: the oracle's column maxima with the reference's signed
lazy-F exit against the same with the exit made unsigned, above the unit's threshold.  GPU only."""
import ctypes
import os

import pytest

import helpers
import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

SEG = 5000
ENC = 22                      # one-to-one, read forwards: unit column = DNA position
ENC_REV = 23                  # one-to-one, read backwards
BACKGROUND = {ENC: 4, ENC_REV: 0}    # q2cat segment under the plants (one in which the gapped plant itself stays below 251)
Q2_BOUNDARY = 15              # the gapped plant sits at stripe boundary 15: virtual lanes 120 / 121
GAP_COLUMN = 2016             # first column of the gapped plant (picked for test_cut_is_proven_before_the_taints_are_set)
OVERFLOW_ROWS = (0, 51)       # query rows of the overflow plant: 51 x 5 = 255, first cell >= 251 in row 50 (virtual lane 2)
OVERFLOW_LANE = 50 // 22
MIN_OVERFLOW_THR = 204        # (int)(0.8 * 255): the lowest threshold of a unit that holds an overflow
SKEW_DISTANCES = (1, 63, 64, 127, 128)
COUNTERS = ("units", "candidates", "align_calls", "hazard_units", "stage2_overflow_units", "stage1_word_reruns")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def h19(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]


@pytest.fixture(scope="module")
def q2cat(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "q2cat.fa"))[1]


@pytest.fixture(scope="module")
def orc(oracle_build):
    o = helpers.Oracle(oracle_build)
    o.lib.fo_pre_align_noq2.restype = None
    o.lib.fo_pre_align_noq2.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return o


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def put(dna, enc, col, rows):
    """write the exact pre-image of the query rows `rows` so that the unit of encoding enc reads them from column col on"""
    tract = helpers.preimage(rows, enc, synth._Rng(1000 * enc + col))
    assert tract is not None
    pos = len(dna) - col - len(tract) if synth.enc_reversed(enc) else col
    assert 0 <= pos and pos + len(tract) <= len(dna)
    dna[pos:pos + len(tract)] = tract


def gap_plant_rows(rna, j):
    b = j * ((len(rna) + 15) // 16)
    return rna[b - 48:b] + rna[b + 26:b + 47]


def overflow_rows(rna, rows=OVERFLOW_ROWS):
    return rna[rows[0]:rows[1]]


def both_maxima(orc, rna, dna, enc):
    """the oracle's column maxima of the unit: (with the reference's signed exit, with the exit made unsigned, threshold)"""
    t, _ = orc.encode_unit(bytes(dna), enc)
    ref = orc.pre_align(rna, t)
    buf = (ctypes.c_int * len(t))()
    orc.lib.fo_pre_align_noq2(rna, len(rna), t, len(t), buf)
    return ref, list(buf), int(orc.stage1_max(rna, t) * 0.8)


def cut_of(cols):
    """the overflow cut of a row of column maxima as the byte kernel leaves it: everything from the cut on is zero"""
    c = len(cols)
    while c > 0 and cols[c - 1] == 0:
        c -= 1
    return c


def q2_columns(ref, noq2, thr):
    return [c for c in range(len(ref)) if ref[c] != noq2[c] and (ref[c] > thr or noq2[c] > thr)]


def q2_site(orc, rna, q2cat, base, enc, gap_col=GAP_COLUMN):
    """A q2cat segment with the gapped plant under encoding enc at column gap_col, and the last column at which Q2 matters under a
    threshold of 204."""
    dna = bytearray(q2cat[base * SEG:(base + 1) * SEG])
    put(dna, enc, gap_col, gap_plant_rows(rna, Q2_BOUNDARY))
    ref, noq2, _ = both_maxima(orc, rna, dna, enc)
    cols = q2_columns(ref, noq2, MIN_OVERFLOW_THR)
    assert cols and cut_of(ref) == SEG and cut_of(noq2) == SEG, (base, enc, cols[:3], cut_of(ref), cut_of(noq2))
    assert gap_col + 48 <= cols[0] and cols[-1] < gap_col + 400
    return dna, cols[-1]


def with_overflow(orc, rna, dna, enc, col):
    """dna with the overflow plant from unit column col on; checks that the unit's cut is the plant's 51st column, in both variants"""
    out = bytearray(dna)
    put(out, enc, col, overflow_rows(rna))
    ref, noq2, thr = both_maxima(orc, rna, out, enc)
    assert cut_of(ref) == col + 50 and cut_of(noq2) == col + 50 and ref[col + 49] == 250, (enc, col, cut_of(ref), cut_of(noq2), ref[col + 49])
    return bytes(out), q2_columns(ref, noq2, thr)


# ---- scans ----------------------------------------------------------------------------------------------------------------------
def oracle_records(oracle_build, tmp, name, rna, dna):
    rna_fa, dna_fa = os.path.join(str(tmp), name + "_q.fa"), os.path.join(str(tmp), name + "_d.fa")
    synth.write_fasta(rna_fa, name, rna)
    synth.write_fasta(dna_fa, f"syn|chrP|1-{len(dna)}", dna)
    meta, units = helpers.parse_scan(helpers.oracle_cli(oracle_build, "scan", rna_fa, dna_fa, "-threads", "8"))
    assert meta["m"] == len(rna)
    return units


def scan(mod, rna, dna, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_query(rna)
    r = e.scan(dna, mod.default_params(cLength=20))          # cLength == ntMin: LongTarget's tail filter == fastSIM's
    out = {"trips": r.triplexes(), "recs": r.recs, "pool": r.pool, "stats": {k: r.stats[k] for k in COUNTERS}, "all": r.stats}
    del r
    e.close()
    return out


def both_settings(mod, rna, dna, units, what, **options):
    """scans with q2_past_cut 0 and 1: each gives the oracle's records, and they agree in records, pools and counters"""
    want = helpers.expected_triplexes(units)
    got = [scan(mod, rna, dna, q2_past_cut=v, **options) for v in (0, 1)]
    print(f"{what}: {len(want)} triplexes, counters {got[0]['stats']}, k_scan {got[0]['all']['kernel_ms'][0]:.3f} / {got[1]['all']['kernel_ms'][0]:.3f} ms")
    for v in (0, 1):
        assert got[v]["trips"] == want, (what, "q2_past_cut", v)
        assert got[v]["stats"]["units"] == len(units) and got[v]["stats"]["candidates"] == sum(u["ncand"] for u in units), (what, v)
    assert got[0]["recs"] == got[1]["recs"] and got[0]["pool"] == got[1]["pool"], what
    assert got[0]["stats"] == got[1]["stats"], (what, got[0]["stats"], got[1]["stats"])
    return got[0]["stats"]


@pytest.fixture(scope="module")
def cases(orc, oracle_build, h19, q2cat, tmp_path_factory):
    """name -> (DNA, the oracle's units, the (segment, encoding) units in which Q2 matters), each computed once and left unchanged"""
    tmp = tmp_path_factory.mktemp("q2_past_cut")
    cache = {}

    def get(name, build):
        if name not in cache:
            dna = build()
            cache[name] = (dna, oracle_records(oracle_build, tmp, name, h19, dna), helpers.q2_units_that_matter(orc, h19, dna))
        return cache[name]

    return get


def _skew_case(orc, h19, q2cat, enc, d):
    """the overflow plant starts d columns after the last column at which Q2 matters"""
    dna, qlast = q2_site(orc, h19, q2cat, BACKGROUND[enc], enc)
    out, cols = with_overflow(orc, h19, dna, enc, qlast + d)
    assert cols                                                          # Q2 still matters under the unit's new threshold
    return out, qlast


def _before_case(orc, h19, q2cat, enc):
    """the overflow plant ends more than 200 columns before the first column of the Q2 site"""
    dna, _ = q2_site(orc, h19, q2cat, BACKGROUND[enc], enc)
    out, cols = with_overflow(orc, h19, dna, enc, GAP_COLUMN - 300)
    assert not cols                                                      # the site lies behind the cut: it cannot matter
    return out


# ---- 1 and 6: the cut lies before the Q2 site -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dp_f16", [1, 0])
@pytest.mark.parametrize("enc", [ENC, ENC_REV])
def test_cut_before_the_q2_site(mod, orc, h19, q2cat, cases, enc, dp_f16):
    """The tracking is already off when the pipeline reaches the Q2 site, and nothing may depend on it: the site's columns lie
    behind the cut."""
    dna, units, matter = cases(f"before_{enc}", lambda: _before_case(orc, h19, q2cat, enc))
    assert (0, enc) not in matter
    st = both_settings(mod, h19, dna, units, f"cut before the site, enc {enc}, dp_f16 {dp_f16}", dp_f16=dp_f16)
    assert st["stage2_overflow_units"] >= 1 and st["hazard_units"] >= len(matter)


# ---- 2, 3 and 6: the cut lies right behind the Q2 site --------------------------------------------------------------------------
@pytest.mark.parametrize("dp_f16", [1, 0])
@pytest.mark.parametrize("enc,d", [(ENC, d) for d in SKEW_DISTANCES] + [(ENC_REV, 1), (ENC_REV, 64)])
def test_cut_right_behind_the_q2_site(mod, orc, h19, q2cat, cases, enc, d, dp_f16):
    """The overflow plant starts d columns after the last column at which Q2 matters: the pipeline skew (lane 2 proves the cut while
    lanes 120 / 121 are still on columns before it) and both sides of a block boundary.  Switching off too early loses the unit's
    hazard flag."""
    made = {}

    def build():
        made["dna"], made["qlast"] = _skew_case(orc, h19, q2cat, enc, d)
        return made["dna"]

    dna, units, matter = cases(f"skew_{enc}_{d}", build)
    assert (0, enc) in matter, (enc, d, matter)
    st = both_settings(mod, h19, dna, units, f"cut {d} columns behind the site, enc {enc}, dp_f16 {dp_f16}", dp_f16=dp_f16)
    assert st["hazard_units"] >= len(matter) >= 1 and st["stage2_overflow_units"] >= 1


def test_cut_is_proven_before_the_taints_are_set(orc, h19, q2cat):
    """The geometry that test_cut_right_behind_the_q2_site rests on, from the oracle's column maxima alone: at the first distance
    the block of 64 steps in which the overflow's first cell >= 251 is computed closes before lanes 120 / 121 reach the columns of
    the gapped plant in which the taints are set, and those are reached less than 128 steps later."""
    dna, qlast = q2_site(orc, h19, q2cat, BACKGROUND[ENC], ENC)
    proven_at = qlast + SKEW_DISTANCES[0] + 50 + OVERFLOW_LANE            # pipeline step of the first cell >= 251
    block_closes = proven_at | 63
    taints_set_at = GAP_COLUMN + 47 + 8 * Q2_BOUNDARY                     # F crosses the boundary in the plant's 48th column
    assert block_closes < taints_set_at < block_closes + 128, (qlast, proven_at, block_closes, taints_set_at)


# ---- 3: the overflow's first cell >= 251 at a block edge ------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [63, 0, 1])
def test_overflow_at_a_block_edge(mod, orc, h19, q2cat, cases, edge):
    """The first cell >= 251 is computed in the last step of a 64-step block, in the first step of the next and one step later (the
    plant moves by one column each time), behind the Q2 site of the skew cases."""

    def build():
        dna, qlast = q2_site(orc, h19, q2cat, BACKGROUND[ENC], ENC)
        col = qlast + 130
        col += (edge - (col + 50 + OVERFLOW_LANE)) % 64
        assert (col + 50 + OVERFLOW_LANE) % 64 == edge
        return with_overflow(orc, h19, dna, ENC, col)[0]

    dna, units, matter = cases(f"edge_{edge}", build)
    st = both_settings(mod, h19, dna, units, f"first cell >= 251 at step = {edge} mod 64")
    assert st["hazard_units"] >= len(matter) and st["stage2_overflow_units"] >= 1


# ---- 4: a tainted maximum must not trigger --------------------------------------------------------------------------------------
def test_tainted_maximum_does_not_prove_a_cut(mod, orc, h19, q2cat, cases):
    """None of the 19 q2cat segments holds a unit whose first maximum >= 251 is tainted (their Q2 sites end below 251), so one is
    built by letting a Q2 site's alignment run past 251: under encoding 23 the gapped plant in segment 8 runs on into the bases
    behind it, the textbook recurrence reaches 251 at a column where the reference, which lost the 124 of the vertical gap, holds
    less and never overflows.  The unit must be re-run on the stripe-faithful kernel, whatever the option says."""

    def build():
        dna = bytearray(q2cat[8 * SEG:9 * SEG])
        put(dna, ENC_REV, 2000, gap_plant_rows(h19, Q2_BOUNDARY))
        ref, noq2, thr = both_maxima(orc, h19, dna, ENC_REV)
        c = cut_of(noq2)
        assert c < SEG and cut_of(ref) == SEG and 0 < ref[c] < 251, (c, cut_of(ref), ref[c])
        assert q2_columns(ref, noq2, thr)
        return bytes(dna)

    dna, units, matter = cases("tainted", build)
    assert (0, ENC_REV) in matter
    st = both_settings(mod, h19, dna, units, "tainted first maximum >= 251")
    assert st["hazard_units"] >= len(matter) >= 1


# ---- 5: several query tiles -----------------------------------------------------------------------------------------------------
def test_three_query_tiles(mod, oracle_build, golden_dir, tmp_path_factory):
    """MALAT1 (8 708 rows: stripes of 545 rows, 24 virtual lanes each, three tiles of 128 virtual lanes).  The overflow plant reads
    rows [4000, 4051), in the second tile only; a gapped plant at stripe boundary 12 (third tile) comes 130 columns before it, so
    that chain state crosses a tile boundary before the second tile's pass proves the cut."""
    _, rna = synth.read_fasta(os.path.join(golden_dir, "MALAT1.fa"))
    seg = (len(rna) + 15) // 16
    vs = 8 * ((seg + 191) // 192)
    assert vs // 8 == 3 and 128 * seg // vs <= 4000 and 4051 <= 256 * (seg // vs)      # rows of virtual lanes [128, 256)
    dna = bytearray(synth.random_dna(SEG, 2201))
    put(dna, ENC, 1500, gap_plant_rows(rna, 12))
    put(dna, ENC, 1700, overflow_rows(rna, (4000, 4051)))
    dna = bytes(dna)
    units = oracle_records(oracle_build, tmp_path_factory.mktemp("q2_past_cut_tiles"), "tiles", rna, dna)
    st = both_settings(mod, rna, dna, units, "three query tiles")
    assert st["stage2_overflow_units"] >= 1


# ---- 7: both settings on plain input --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "genome"])
@pytest.mark.parametrize("dp_f16", [1, 0])
def test_both_settings_on_plain_dna(mod, h19, kind, dp_f16):
    """200 kb of random and of chromosome-like DNA: identical records, pools and counters; about 7 % of the units hold an overflow."""
    dna = synth.random_dna(200_000, 31337) if kind == "random" else synth.genome_like(200_000, 31337, soft_mask=False)
    got = [scan(mod, h19, dna, q2_past_cut=v, dp_f16=dp_f16) for v in (0, 1)]
    print(f"{kind}, dp_f16 {dp_f16}: {len(got[0]['trips'])} triplexes, counters {got[0]['stats']}")
    assert got[0]["recs"] == got[1]["recs"] and got[0]["pool"] == got[1]["pool"]
    assert got[0]["stats"] == got[1]["stats"]
    assert got[0]["stats"]["stage2_overflow_units"] > 0
