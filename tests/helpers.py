"""Shared helpers for the test-suite (probe line protocol, oracle ctypes binding, inputs)."""
import ctypes
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
REF_FASIM = os.path.join(ROOT, "oracle", "_ref", "fasim_ref")


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def oracle_cli(build_dir, *args):
    exe = os.path.join(build_dir, "fasim_oracle")
    return subprocess.run([exe, *args], check=True, stdout=subprocess.PIPE).stdout


class Oracle:
    """ctypes view of oracle/_build/libfasim_oracle.so (CHECKER ONLY)."""

    def __init__(self, build_dir):
        self.lib = ctypes.CDLL(os.path.join(build_dir, "libfasim_oracle.so"))
        L = self.lib
        L.fo_stage1_max.restype = ctypes.c_int
        L.fo_stage1_max.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.fo_pre_align.restype = None
        L.fo_pre_align.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.fo_pick_candidates.restype = ctypes.c_int
        L.fo_pick_candidates.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        L.fo_align.restype = ctypes.c_int
        L.fo_align.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                               ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
        L.fo_sim_forward_nodes.restype = ctypes.c_int
        L.fo_sim_forward_nodes.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_long,
                                           ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.fo_encode_unit.restype = None
        L.fo_encode_unit.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]

    def stage1_max(self, q: bytes, t: bytes) -> int:
        return self.lib.fo_stage1_max(q, len(q), t, len(t))

    def pre_align(self, q: bytes, t: bytes):
        out = (ctypes.c_int * len(t))()
        self.lib.fo_pre_align(q, len(q), t, len(t), out)
        return list(out)

    def candidates(self, cols, thr):
        n = len(cols)
        arr = (ctypes.c_int * n)(*cols)
        s = (ctypes.c_int * (n + 1))()
        p = (ctypes.c_int * (n + 1))()
        k = self.lib.fo_pick_candidates(arr, n, thr, s, p, n + 1)
        return [(s[i], p[i]) for i in range(k)]

    def align(self, q: bytes, w: bytes):
        out5 = (ctypes.c_int * 5)()
        cig = (ctypes.c_uint32 * 4096)()
        k = self.lib.fo_align(q, len(q), w, len(w), out5, cig, 4096)
        assert k >= 0
        return tuple(out5), cigar_to_string(cig[:k])

    def align_ex(self, q: bytes, w: bytes):
        """align plus the oracle's `tainted` flag (the reference's traceback reads memory it never wrote: no defined answer) and
        the band widths its banded_sw went through: ((score, ref_begin, ref_end, q_begin, q_end), CIGAR, tainted, bands)"""
        L = self.lib
        L.fo_align_ex.restype = ctypes.c_int
        L.fo_align_ex.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        out5, cig = (ctypes.c_int * 5)(), (ctypes.c_uint32 * 4096)()
        tainted, bands, nb = ctypes.c_int(0), (ctypes.c_int * 32)(), ctypes.c_int(0)
        k = L.fo_align_ex(q, len(q), w, len(w), out5, cig, 4096, ctypes.byref(tainted), bands, 32, ctypes.byref(nb))
        assert k >= 0 and nb.value <= 32
        return tuple(out5), cigar_to_string(cig[:k]), bool(tainted.value), list(bands[:nb.value])

    def sim_forward_nodes(self, q: bytes, t: bytes, min_score: int):
        """node list after the first sweep of SIM() (oracle/fasim_sim_oracle.cpp), as 9-tuples in list order"""
        out = (ctypes.c_long * (9 * 50))()
        k = self.lib.fo_sim_forward_nodes(q, len(q), t, len(t), min_score, out, 50)
        return [tuple(out[9 * x + y] for y in range(9)) for x in range(k)]

    def encode_unit(self, seg: bytes, enc: int):
        t = ctypes.create_string_buffer(len(seg))
        s = ctypes.create_string_buffer(len(seg) + 1)
        self.lib.fo_encode_unit(seg, len(seg), enc, t, s)
        return t.raw[:len(seg)], s.raw[:len(seg)].rstrip(b"\0")


def cigar_to_string(cigar):
    ops = "MIDNSHP=X"
    return "".join(f"{c >> 4}{'M' if (c & 15) > 8 else ops[c & 15]}" for c in cigar)


def parse_scan(text: bytes):
    """ref_probe/fasim_oracle `scan` protocol -> list of unit dicts (see oracle/ref_probe.cpp)."""
    units, cur, cand = [], None, None
    meta = {}
    for line in text.decode().splitlines():
        f = line.split(" ")
        k = f[0]
        if k == "Q":
            meta = {"m": int(f[1]), "dna_len": int(f[2]), "nseg": int(f[3]), "skipped": []}
        elif k == "K":
            meta["skipped"].append(int(f[1]))
        elif k == "U":
            cur = {"seg": int(f[1]), "enc": int(f[2]), "dna_start": int(f[3]), "strand": int(f[4]), "para": int(f[5]),
                   "rule": int(f[6]), "n": int(f[7]), "stage1": int(f[8]), "thr": int(f[9]), "colhash": f[10],
                   "nhits": int(f[11]), "ncand": int(f[12]), "hits": [], "cands": [], "triplexes": []}
            units.append(cur)
        elif k == "H":
            cur["hits"].append((int(f[1]), int(f[2])))
        elif k == "C":
            cand = {"score": int(f[1]), "pos": int(f[2]), "tries": []}
            cur["cands"].append(cand)
        elif k == "T":
            cand["tries"].append({"it": int(f[1]), "L": int(f[2]), "score": int(f[3]), "ref_begin": int(f[4]),
                                  "ref_end": int(f[5]), "q_begin": int(f[6]), "q_end": int(f[7]), "cigar": f[8]})
        elif k == "X":
            cur["triplexes"].append(tuple(f[1:]))
    return meta, units


def fnv1a_ints(vals):
    h = 1469598103934665603
    for v in vals:
        x = v & 0xFFFFFFFF
        for b in range(4):
            h ^= (x >> (8 * b)) & 0xFF
            h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def probe_random_vectors():
    """Seeded raw-kernel vectors: a ~900-nt query, 40 planted targets (S and P requests) and 40 windows (A requests).
    The reference probe's answers are stored in tests/golden/probe_rnd40.rsp.gz (`make_golden.py probe`)."""
    import synth
    rng = synth._Rng(424242)
    q = synth.random_rna(900 + rng.below(50), 7).decode()
    reqs, targets, wins = [], [], []
    for k in range(40):
        t = synth.planted_dna(300 + rng.below(900), 1000 + k, q.encode(), every=150, max_len=120).decode()
        targets.append(t.encode())
        reqs += [f"S {q} {t}", f"P {q} {t}"]
        w = t[:60 + rng.below(130)]
        wins.append(w.encode())
        reqs.append(f"A {q} {w}")
    return q.encode(), targets, wins, reqs


# ---- untidy queries: U, lower case, N and IUPAC letters (test_oracle_golden.py, test_gpu_dirty_query.py) ------------------------
# The four query classes of DESIGN section 7: k_striped only, systolic with the coarse hazard test, one tile, two tiles.
DIRTY_LENGTHS = (100, 700, 1300, 4000)
DIRTY_DNA_LEN = 10000
# query seeds (the DNA takes seed + 1), picked among a few so that the conditions of test_dirty_query_scan_and_input_conditions hold
DIRTY_SEEDS = {100: 9101, 700: 9110, 900: 9109, 1300: 9120, 4000: 9145}
DIRTY_Q2_UNITS = {1300: 3, 4000: 2}     # hazard (Q2) units that matter, by q2_units_that_matter (test_oracle_golden.py holds the oracle to it)
# (segment, encoding) of the plants, all under encodings that give every query letter a pre-image (22, 23, 26, 27, 40, 41).  Plants
# of one strength share a unit: the unit's threshold is 0.8 times its best stage-1 score.
DIRTY_STAGE2_UNITS = ((0, 26), (0, 27), (1, 26), (1, 27), (0, 22), (1, 23))     # 30-row plants (150)
DIRTY_STAGE1_UNITS = ((0, 40), (1, 41), (1, 40))                                # 44-row plants (220), read in full by stage 1 only
DIRTY_GAP_UNITS = ((0, 41), (0, 23), (1, 22))                                   # gapped plants (240 and 105)


def dirty_zones(m):
    """((first, end) of the U stretch, (first, end) of the lower-case stretch, first row of the last third)."""
    w = max(1, m // 6)
    return (m // 12, m // 12 + w), (m // 3, m // 3 + w), 2 * m // 3


def dirty_query(m, seed):
    """A seeded random query with three untidy zones: a stretch of m / 6 rows in which every T is written U, a stretch of m / 6
    rows in lower case, and a last third with one letter of N R Y n u every 23 ... 52 rows."""
    import synth
    q = bytearray(synth.random_rna(m, seed))
    (u0, u1), (l0, l1), s0 = dirty_zones(m)
    for i in range(u0, u1):
        if q[i] == ord("T"):
            q[i] = ord("U")
    q[l0:l1] = bytes(q[l0:l1]).lower()
    rng = synth._Rng(seed * 31 + 7)
    i = s0 + rng.below(23)
    while i < m:
        q[i] = b"NRYnu"[rng.below(5)]
        i += 23 + rng.below(30)
    return bytes(q)


def dirty_rows(query):
    """{'U': rows of the U stretch that hold a U, 'lower': rows of the lower-case stretch, 'N': untidy rows of the last third}."""
    (u0, u1), (l0, l1), s0 = dirty_zones(len(query))
    return {"U": [i for i in range(u0, u1) if query[i] == ord("U")], "lower": list(range(l0, l1)),
            "N": [i for i in range(s0, len(query)) if query[i] in b"NRYnu"]}


def dirty_reading(rows: bytes, stage, rng, avoid=b""):
    """Query rows as a stage reads them, in upper-case ACGT: stage 1 reads U as T, stages 2 and 3 read U as A (the reference's
    quirk); a letter that matches nothing (N, R, Y) is filled arbitrarily, with no letter of `avoid`."""
    fill = bytes(c for c in b"ACGT" if c not in avoid)
    out = bytearray()
    for c in rows.upper():
        if c == ord("U"):
            c = ord("T") if stage == 1 else ord("A")
        elif c not in b"ACGT":
            c = fill[rng.below(len(fill))]
        out.append(c)
    return bytes(out)


def dirty_windows(query, rows, lo_bound, hi_bound, need, most, length=30):
    """Up to three windows [lo, lo + length) within [lo_bound, hi_bound) that hold between `need` and `most` of `rows` and whose
    stage-2 reading has no G next to a G, at least `length` / 3 apart.
    (Under the one-to-one encodings a query G is written by a T of the strand that the triplex record shows, and two T in a row
    there cost the record 1 000 of stability, penaltyT: such a hit is found and aligned but never becomes a triplex.)"""
    import synth
    rowset, out = set(rows), []
    for lo in range(max(0, lo_bound), min(len(query), hi_bound) - length + 1):
        held = sum(r in rowset for r in range(lo, lo + length))
        text = dirty_reading(query[lo:lo + length], 2, synth._Rng(1), avoid=b"G")
        if need <= held <= most and b"GG" not in text and (not out or lo - out[-1][0] >= length // 3):
            out.append((lo, lo + length))
    return out[:3] if len(out) <= 3 else [out[0], out[len(out) // 2], out[-1]]


def dirty_dna(query, n, seed, with_plants=False):
    """DNA for an untidy query: synth.planted_dna (which leaves lower-case and N rows to chance), then exact pre-images of query
    windows, one every 230 nt in the first two segments, under the one-to-one encodings:
      kind 'U', 'lower', 'N': 30-row windows (dirty_windows) that hold rows of the U stretch, 4 ... 9 rows of the lower-case stretch
          (the triplex record counts a lower-case row as a mismatch: more of them and its identity falls below 60) or an untidy
          row of the last third, as stages 2 and 3 read them (case folded, U as A), each in several units of DIRTY_STAGE2_UNITS:
          their diagonals cross the untidy rows, and the triplexes they give overlap them;
      kind 'stage1': 44-row windows around the U stretch as stage 1 reads them (U as T), in the units of DIRTY_STAGE1_UNITS: stage 1
          sees up to 220 there, stage 2 a mismatch at every U, so the threshold 0.8 * stage 1 comes from a diagonal that stage 2
          scores lower (windows with few U keep a candidate) or loses (windows inside the stretch);
      kind 'gap' (queries of 1 300 rows and more): the construction of ROW_LAYOUT_GAP_PLANTS at stripe boundaries b of the last
          third whose 26 gap rows [b, b + 26) hold an untidy letter, so that the vertical gap of a hazard (Q2) unit runs through it.
    Two bases on either side of a 30-row plant mismatch the query, so that the hit rarely grows beyond it.
    with_plants: also the list of plants (kind, seg, enc, lo, hi, pos, n)."""
    import synth
    m = len(query)
    rng = synth._Rng(seed * 131 + 5)
    dna = bytearray(synth.planted_dna(n, seed, query, every=400, min_len=25, max_len=36, mut_pct=8))
    rows = dirty_rows(query)
    (u0, u1), (l0, l1), s0 = dirty_zones(m)
    L = 30
    wanted = {"U": dirty_windows(query, rows["U"], u0 - L, u1 + L, 1, 6, L),
              "lower": dirty_windows(query, rows["lower"], l0 - L, l0 + 9, 4, 9, L) + dirty_windows(query, rows["lower"], l1 - 9, l1 + L, 4, 9, L),
              "N": dirty_windows(query, rows["N"], s0 - L, m, 1, 2, L)}
    slots = {0: 0, 1: 0}
    plants = []

    def put(kind, unit, lo, hi, tract):
        s, enc = unit
        pos = 4900 * s + 200 + 230 * slots[s]
        slots[s] += 1
        assert pos + len(tract) <= 4900 * s + 4800 and pos + len(tract) <= n, (kind, unit, pos)
        dna[pos:pos + len(tract)] = tract
        plants.append({"kind": kind, "seg": s, "enc": enc, "lo": lo, "hi": hi, "pos": pos, "n": len(tract)})

    def other(row):
        """a letter that row `row` of the query does not match in stage 2, and no G"""
        if not 0 <= row < m:
            return b"A"
        c = dirty_reading(query[row:row + 1], 2, rng, avoid=b"G")
        return bytes([next(x for x in b"ACT" if x != c[0])])

    seg = (m + 15) // 16
    if m >= 1300:
        untidy, gaps = rows["N"], []
        for j in range(1, 16):
            b = j * seg
            if b + 47 <= m and any(b <= r < b + 26 for r in untidy):
                gaps.append((any(b - 48 <= r < b or b + 26 <= r < b + 47 for r in untidy), j))
        for unit, (_, j) in zip(DIRTY_GAP_UNITS, sorted(gaps)):
            lo = j * seg - 48
            put("gap", unit, lo, lo + 95, preimage(dirty_reading(query[lo:lo + 48] + query[lo + 74:lo + 95], 2, rng), unit[1], rng))
    for ki, kind in enumerate(("U", "lower", "N")):
        ws = wanted[kind]
        for j in range(min(9, 6 * len(ws))):
            w = j % len(ws)
            unit = DIRTY_STAGE2_UNITS[(j // len(ws) + w + 2 * ki) % 6]
            lo, hi = ws[w]
            text = other(lo - 2) + other(lo - 1) + dirty_reading(query[lo:hi], 2, rng, avoid=b"G") + other(hi) + other(hi + 1)
            put(kind, unit, lo, hi, preimage(text, unit[1], rng))
    W = min(44, m)
    for t in range(6):
        lo = max(0, min(u0 - 38 + t * (u1 - u0 + 32) // 5, m - W))
        unit = DIRTY_STAGE1_UNITS[t % len(DIRTY_STAGE1_UNITS)]
        put("stage1", unit, lo, lo + W, preimage(dirty_reading(query[lo:lo + W], 1, rng), unit[1], rng))
    assert len(dna) == n
    return (bytes(dna), plants) if with_plants else bytes(dna)


def dirty_case(m):
    """(query, DNA) of the untidy-query case of m rows."""
    q = dirty_query(m, DIRTY_SEEDS[m])
    return q, dirty_dna(q, DIRTY_DNA_LEN, DIRTY_SEEDS[m] + 1)


DIRTY_DNA_HEADER = "syn|chrD|1-%d" % DIRTY_DNA_LEN


def dirty_case_files(tmp_dir, m):
    """The case of m rows written as FASTA: (query path, DNA path, query, DNA)."""
    import synth
    rna, dna = dirty_case(m)
    rna_fa, dna_fa = os.path.join(str(tmp_dir), f"dirtyq_{m}.fa"), os.path.join(str(tmp_dir), f"dirtyq_{m}_dna.fa")
    synth.write_fasta(rna_fa, f"dirtyq_{m}", rna)
    synth.write_fasta(dna_fa, DIRTY_DNA_HEADER, dna)
    return rna_fa, dna_fa, rna, dna


def triplex_rows_overlap(x, rows):
    """Does the X line x (parse_scan) cover one of the query rows (0-based)?  Its first two fields are the 1-based query range."""
    a, b = sorted((int(x[0]), int(x[1])))
    return any(a - 1 <= r <= b - 1 for r in rows)


def q2_units_that_matter(orc, rna, dna, cut=5000, step=4900):
    """(segment, encoding) of the units in which the reference's signed lazy-F exit changes a column maximum above the unit's
    threshold: the oracle's pre_align against the same with the exit made unsigned (the criterion of
    test_gpu_parity._q2_units_that_matter, on the segments as the scan cuts them)."""
    orc.lib.fo_pre_align_noq2.restype = None
    orc.lib.fo_pre_align_noq2.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    out = []
    for s, start in enumerate(range(0, max(1, len(dna) - (cut - step)), step)):
        for enc in range(48):
            t, _ = orc.encode_unit(dna[start:start + cut], enc)
            ref = orc.pre_align(rna, t)
            buf = (ctypes.c_int * len(t))()
            orc.lib.fo_pre_align_noq2(rna, len(rna), t, len(t), buf)
            if ref == list(buf):
                continue
            thr = int(orc.stage1_max(rna, t) * 0.8)
            if [(c, v) for c, v in enumerate(ref) if v > thr] != [(c, v) for c, v in enumerate(buf) if v > thr]:
                out.append((s, enc))
    return out


def probe_dirty_vectors():
    """probe_random_vectors for an untidy query: the 900-nt dirty query, 40 targets planted with it (S and P requests; every fourth
    holds N and lower-case letters) and 40 windows (A requests).  The reference probe's answers: tests/golden/probe_dirty40.rsp.gz
    (`make_golden.py dirtyq`)."""
    import synth
    rng = synth._Rng(515151)
    q = dirty_query(900, DIRTY_SEEDS[900])
    rows = dirty_rows(q)
    marks = rows["U"][::8] + rows["lower"][::12] + rows["N"]
    reqs, targets, wins = [], [], []
    for k in range(40):
        t = bytearray(synth.planted_dna(300 + rng.below(900), 2000 + k, q, every=150, max_len=120))
        # exact stage-2 and stage-1 readings of a window around an untidy row, forwards (a raw target is not rule-encoded)
        for stage, at in ((2, 20), (1, 160)):
            r = marks[rng.below(len(marks))]
            lo = max(0, min(r - 10 - rng.below(25), len(q) - 44))
            t[at:at + 44] = dirty_reading(q[lo:lo + 44], stage, rng)
        if k % 4 == 3:
            for _ in range(6):
                i = rng.below(len(t))
                t[i] = b"Nnacgt"[rng.below(6)] if t[i] != ord("A") else ord("a")
        t = bytes(t)
        targets.append(t)
        reqs += [f"S {q.decode()} {t.decode()}", f"P {q.decode()} {t.decode()}"]
        w = t[:60 + rng.below(130)]
        wins.append(w)
        reqs.append(f"A {q.decode()} {w.decode()}")
    return q, targets, wins, reqs


def syn10k_ntmax_inputs():
    """BASELINE config 5 in miniature: a 10 kb synthetic lncRNA and 12 kb of DNA planted with it (byte overflows, 16-bit
    re-runs).  The reference probe's `scan -detail 0 -na 1000` of them: tests/golden/syn10k_na1000.scan.gz."""
    import synth
    rna = synth.random_rna(10000, 515)
    dna = synth.planted_dna(12000, 516, rna, every=500, max_len=180, mut_pct=6)
    return rna, dna


def have_ref_probe():
    return os.access(REF_PROBE, os.X_OK)


def ref_batch(requests):
    """Run the compiled reference probe (if present) on S/P/K/A request lines."""
    req = ("\n".join(requests) + "\n").encode()
    out = subprocess.run([REF_PROBE, "batch"], input=req, check=True, stdout=subprocess.PIPE).stdout
    return out.decode().splitlines()


def expected_triplexes(units):
    """The X lines of parsed `scan` units as ScanResult.triplexes() tuples (identity / stability as float bits)."""
    exp = []
    for u in units:
        for x in u["triplexes"]:
            f = list(x)
            exp.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]),
                        int(f[9], 16), int(f[10], 16), f[11].encode(), f[12].encode(), u["seg"], u["enc"]))
    return exp


def fnv1a_rows(rows):
    """fnv1a_ints of every row (the `colhash` of the scan protocol), vectorised over the rows with numpy."""
    import numpy as np
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    width = int(lens.max()) if len(rows) else 0
    a = np.zeros((len(rows), width), dtype=np.uint64)
    for i, r in enumerate(rows):
        a[i, :len(r)] = np.asarray(r, dtype=np.int64).astype(np.uint32)
    h = np.full(len(rows), 1469598103934665603, dtype=np.uint64)
    prime, mask = np.uint64(1099511628211), np.uint64(0xFF)
    for c in range(width):
        live = lens > c
        x, g = a[:, c], h
        for b in range(4):
            g = (g ^ ((x >> np.uint64(8 * b)) & mask)) * prime
        h = np.where(live, g, h)
    return [f"{int(v):016x}" for v in h]


def unit_summary_digest(units):
    """One record's units in scan order, each (enc, stage1, thr, colhash hex, ncand), folded with fnv1a_ints."""
    vals = []
    for enc, s1, thr, colhash, ncand in units:
        ch = int(colhash, 16)
        vals += [enc, s1, thr, ch & 0xFFFFFFFF, ch >> 32, ncand]
    return fnv1a_ints(vals)


def triplex_digest(trips):
    """SHA-256 prefix of ScanResult.triplexes() tuples (or expected_triplexes() of a fixture), in order."""
    import hashlib
    h = hashlib.sha256()
    for t in trips:
        h.update(" ".join(x.decode() if isinstance(x, bytes) else str(x) for x in t).encode() + b"\n")
    return h.hexdigest()[:16]


def file_digest(data: bytes):
    """(line count, SHA-256 prefix) of an output file, as the peaks manifests store them."""
    import hashlib
    return data.count(b"\n"), hashlib.sha256(data).hexdigest()[:16]


# ---- the reference's 532 MEG3 ChIP peaks (tests/golden/meg3_peaks.fa.gz, `make_golden.py peaks`) ----------------------------
PEAK_QUERIES = ("MEG3", "H19", "MALAT1")
PEAK_FILES = ("TFOsorted", "TFOclass1", "TFOclass2")
MANIFEST_COLUMNS = ("idx", "header", "length", "TFOsorted_lines", "TFOsorted_sha", "TFOclass1_lines", "TFOclass1_sha",
                    "TFOclass2_lines", "TFOclass2_sha", "units", "triplexes", "triplex_sha", "q1", "rev148", "q2")


def read_peaks(path=None):
    """[(header, sequence)] of the peaks file (one sequence line per record)."""
    text = gunzip(path or os.path.join(GOLD, "meg3_peaks.fa.gz"))
    recs, hdr = [], None
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            hdr = line[1:].decode()
        elif line:
            recs.append((hdr, line))
    return recs


def read_manifest(path):
    """peaks_<query>.manifest.gz -> one dict per record (q2 is None where it was not counted)."""
    out = []
    for line in gunzip(path).decode().splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        d = dict(zip(MANIFEST_COLUMNS, f))
        for k in MANIFEST_COLUMNS:
            if k not in ("header", "units", "triplex_sha") and not k.endswith("_sha"):
                d[k] = None if d[k] == "-" else int(d[k])
        out.append(d)
    return out


def split_sections(text: bytes):
    """The `= <idx> <kind> <nbytes>` sections of a peaks detail file -> {(idx, kind): bytes}."""
    out, pos = {}, 0
    while pos < len(text):
        eol = text.index(b"\n", pos)
        _, idx, kind, nbytes = text[pos:eol].decode().split(" ")
        out[(int(idx), kind)] = text[eol + 1:eol + 1 + int(nbytes)]
        pos = eol + 1 + int(nbytes)
    return out


def join_sections(items):
    """Inverse of split_sections: [(idx, kind, bytes)] -> one text."""
    return b"".join(f"= {idx} {kind} {len(data)}\n".encode() + data for idx, kind, data in items)


# ---- the rows-per-lane sweep of the systolic kernels (test_row_layouts_cpu.py, test_gpu_row_layouts.py) -------------------------
# k_scan and k_align_fwd are compiled once per RP = rows per virtual lane, 1 ... 24, and the query length alone picks the build.
# Two single-tile lengths per RP: "full" (every virtual lane owns RP rows, no pad rows) and "ragged" (two lanes of a stripe own RP
# rows, six own RP - 1, 15 zero-score pad rows).  The DNA of a case is generated, never stored.
ROW_LAYOUT_RPS = tuple(range(1, 25))
ROW_LAYOUT_DNA_LEN = 5000
# plants (stripe boundary j, encoding, query rows): 48 rows [b - 42, b + 6) score 240 and stay in the byte range even when both
# neighbours match by chance; 56 rows [b - 50, b + 6) score 280, beyond it (Q1); the rule-1 plants are 32 rows (160) of G / T.  The two long ones come last in their units (the
# odd encodings read the record backwards), so the reference's overflow cut hides no other plant.
ROW_LAYOUT_PLANTS = ((15, 27, 56), (8, 40, 48), (4, 41, 48), (12, 22, 48), (6, 23, 48), (10, 0, 32), (10, 13, 32), (2, 27, 48), (14, 40, 48),
                     (3, 26, 48), (9, 41, 48), (13, 23, 48), (7, 22, 48), (10, 12, 32), (1, 26, 56))
# gapped plants (stripe boundary j, encoding, first DNA base): rows [b - 48, b) and [b + 26, b + 47) back to back.  The best path
# crosses the boundary as a vertical gap: F enters row b at 224 and decays by 4 per row.  The reference's lazy-F loop leaves at
# the row where F is still 128 ... 139 while H - 16 has dropped below 128 (its exit test compares signed bytes: Q2), about 22 rows
# down, so the F = 124 that the second part starts from (124 + 105 = 229, above the unit's threshold) is withheld there: such a
# unit must go to the stripe-faithful re-run, also where the stripes are long enough for the row analysis (seg >= 96).  Each comes
# first in its unit (encoding 23 reads the record backwards), before anything that could reach the overflow cut.
ROW_LAYOUT_GAP_PLANTS = ((5, 40, 280), (11, 23, 4480), (8, 22, 40), (13, 41, 4600), (3, 26, 580), (9, 27, 4700))


def systolic_layout(m):
    """(seg, vs, RP) of a query of m rows: the formula of launch_scan / launch_fwd written out (not imported from the library)."""
    seg = (m + 15) // 16
    vs = 8 * ((seg + 191) // 192)
    return seg, vs, (seg + vs - 1) // vs


def row_layout_cases():
    """[(RP, 'full' | 'ragged', m)]: 48 query lengths from 113 to 3 072."""
    out = []
    for k in ROW_LAYOUT_RPS:
        out.append((k, "ragged", 128 * (k - 1) + 17 if k > 1 else 113))
        out.append((k, "full", 128 * k))
    return out


def row_layout_case_id(case):
    return f"rp{case[0]}-{case[1]}-m{case[2]}"


def band_classes_restated(m):
    """The band heights G of the banded stage 3 that a single-tile query of m rows gets: 8 * G <= 3 * nl, nl = ceil(16 * seg / 48)
    (band.hip; its LDS conditions cannot fail below 3 073 rows)."""
    nl = (16 * ((m + 15) // 16) + 47) // 48
    return [G for G in (8, 16, 32) if 8 * G <= 3 * nl]


def plant_window(m, seg, j, rows=56):
    """Query rows [lo, hi) of a plant of `rows` rows at stripe boundary b = j * seg: six rows beyond b, the others before it, moved
    into the query where it sticks out."""
    b = j * seg
    lo = max(0, min(b + 6 - rows, m - rows))
    return lo, min(m, lo + rows)


def preimage(rows: bytes, enc: int, rng):
    """DNA whose unit of encoding `enc` reads `rows` (None where a row's letter is no output of the rule); a letter with two
    pre-images takes either."""
    import synth
    pre = {}
    for base, o in zip("ATGC", synth.RULE_OUT[enc]):
        pre.setdefault(o, []).append(base)
    if not set(rows.decode()) <= set(pre):
        return None
    tract = bytearray(ord(pre[chr(c)][rng.below(len(pre[chr(c)]))]) for c in rows)
    if synth.enc_reversed(enc):
        tract.reverse()
    return bytes(tract)


def row_layout_inputs(m):
    """(query, DNA record, plants) of the sweep's case of m rows.

    Query: seeded random ACGT, except that 32 rows around boundary 10 are random G / T, the only letters rule 1 can write (its
    four encodings 0, 1, 12, 13 turn A, T, G, C into TGGT or GTTG), so that the rule-1 units hold a real hit too.
    DNA: 5 000 nt of synth.planted_dna (random background with mutated, gapped pre-images of query windows under random encodings),
    then the exact pre-images of ROW_LAYOUT_PLANTS, diagonals that run into a stripe boundary of the reference, one every 300 nt,
    under the one-to-one encodings 22, 23, 26, 27, 40, 41 (odd ones reversed) and under the rule-1 encodings 0, 12 and 13.
    Two more, ROW_LAYOUT_GAP_PLANTS, cross a boundary as a vertical gap.
    plants: dicts enc, j, b (the boundary row), lo, hi (query rows), pos (first DNA base), n, and gap for the last two."""
    import synth
    seg = (m + 15) // 16
    rng = synth._Rng(7700000 + m)
    rna = bytearray(synth.random_rna(m, 7100000 + m))
    lo, hi = plant_window(m, seg, 10, 32)
    for i in range(lo, hi):
        rna[i] = b"GT"[rng.below(2)]
    rna = bytes(rna)
    dna = bytearray(synth.planted_dna(ROW_LAYOUT_DNA_LEN, 7203000 + m, rna, every=150, min_len=35, max_len=70, mut_pct=8))
    plants = []
    for i, (j, enc, rows) in enumerate(ROW_LAYOUT_PLANTS):
        lo, hi = plant_window(m, seg, j, rows)
        tract = preimage(rna[lo:hi], enc, rng)
        assert tract is not None, (m, j, enc)
        pos = 150 + 300 * i
        dna[pos:pos + len(tract)] = tract
        plants.append({"enc": enc, "j": j, "b": j * seg, "lo": lo, "hi": hi, "pos": pos, "n": len(tract)})
    for j, enc, pos in ROW_LAYOUT_GAP_PLANTS:
        lo = max(0, min(j * seg - 48, m - 95))
        tract = preimage(rna[lo:lo + 48] + rna[lo + 74:lo + 95], enc, rng)
        dna[pos:pos + len(tract)] = tract
        plants.append({"enc": enc, "j": j, "b": j * seg, "lo": lo, "hi": lo + 95, "pos": pos, "n": len(tract), "gap": True})
    assert len(dna) == ROW_LAYOUT_DNA_LEN
    return rna, bytes(dna), plants


def oracle_scan_case(build_dir, tmp_dir, m, threads=8):
    """The oracle's `scan` of the case of m rows (default parameters), parsed: (meta, units)."""
    import synth
    rna, dna, _ = row_layout_inputs(m)
    rna_fa, dna_fa = os.path.join(str(tmp_dir), f"q{m}.fa"), os.path.join(str(tmp_dir), f"d{m}.fa")
    synth.write_fasta(rna_fa, f"q{m}", rna)
    synth.write_fasta(dna_fa, f"syn|chrR|1-{len(dna)}", dna)
    return parse_scan(oracle_cli(build_dir, "scan", rna_fa, dna_fa, "-threads", str(threads)))


def q2_units_of_gap_plants(orc, m):
    """Encodings of the gapped plants in whose unit (first segment) the reference's signed lazy-F exit changes a column maximum
    above the unit's threshold: the oracle's pre_align against the same with the exit made unsigned (fo_pre_align_noq2)."""
    orc.lib.fo_pre_align_noq2.restype = None
    orc.lib.fo_pre_align_noq2.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    rna, dna, plants = row_layout_inputs(m)
    out = []
    for enc in sorted({p["enc"] for p in plants if p.get("gap")}):
        t, _ = orc.encode_unit(dna[:ROW_LAYOUT_DNA_LEN], enc)
        ref = orc.pre_align(rna, t)
        buf = (ctypes.c_int * len(t))()
        orc.lib.fo_pre_align_noq2(rna, len(rna), t, len(t), buf)
        thr = int(orc.stage1_max(rna, t) * 0.8)
        if [(c, v) for c, v in enumerate(ref) if v > thr] != [(c, v) for c, v in enumerate(buf) if v > thr]:
            out.append(enc)
    return out


# ---- the storage tiers of the stage-3 finish (test_finish_tiers_cpu.py, test_gpu_finish_tiers.py) -------------------------------
# run_finish (engine_stage3.cpp) offers every alignment to four passes, each handing on what it cannot hold:
#   1  k_finish_lds<64, 2048>     reverse-pass ring of 64 rows, band arrays of 32 entries, 2 048 direction cells
#   2  k_finish_lds<256, 16384>   ring 256, band arrays 128, 16 384 cells
#   3  k_finish, 16 KB of global scratch per alignment (band arrays of at most 256 entries)
#   4  k_finish, 1 MB per alignment (band arrays of at most 4 099 entries)
#   5  the stripe-faithful replay (what no pass holds, and CIGARs of more than 48 runs)
FT_RING_1, FT_BAND_ARRAY_1, FT_CELLS_1 = 64, 32, 2048
FT_RING_2, FT_BAND_ARRAY_2, FT_CELLS_2 = 256, 128, 16384
FT_SLOT_3, FT_WCAP_3 = 16384, 256
FT_SLOT_4, FT_WCAP_4 = 1 << 20, 4099
FT_MAX_RUNS = 48                     # ALIGN_MAX_CIGAR
FT_GAP_OPEN, FT_GAP_EXT = 16, 4
FT_LENGTHS = (1200, 3300)            # one and two systolic tiles
FT_MAX_WINDOW = 200
FT_SEED = 4242
FT_NO_MATCH = b"N" * 24
FT_ONE_GAP = (1, 2, 3, 8, 12, 13, 14, 15, 16, 20, 30, 31, 32, 50, 62, 63, 70, 100)
FT_DOUBLING = (1, 2, 3, 5, 8, 9, 16, 17, 30, 40)


def score_class(score):
    """'lo' (the in-kernel reverse pass), 'mid' (148 ... 250: the exact reverse pass supplies the begin), 'hi' (the 16-bit pass)"""
    return "lo" if score < 148 else "mid" if score < 251 else "hi"


def _ft_sc(a, b):
    return 5 if a == b and a in b"ACGT" else -4


def _ft_ring_overflows(q, w, S, ref_end, read_end, ring):
    """reverse_pass_lds restated: the DP anchored at (read_end, ref_end) walks back column by column and keeps the rows that can
    still reach S (a cell is dropped when its value plus 5 per remaining diagonal step stays below S); True when the live rows
    [lo, hi] of a column, or the row the walk has reached, no longer fit a ring of `ring` entries (device status 2)."""
    NEG = -30000
    R, C = read_end + 1, ref_end + 1
    g0 = _ft_sc(q[read_end], w[ref_end])
    if g0 <= 0 or g0 == S:
        return False
    lo = hi = 0
    G, E = {0: g0}, {0: NEG}
    for j in range(1, C):
        t = w[ref_end - j]
        F = diag = NEG
        nlo = nhi = -1
        if hi - lo + 2 >= ring:
            return True
        i = lo
        while i < R:
            inside = i <= hi
            gp = G.get(i, NEG) if inside else NEG
            ep = E.get(i, NEG) if inside else NEG
            e = max(ep - FT_GAP_EXT, gp - FT_GAP_OPEN)
            g = diag + _ft_sc(q[read_end - i], t) if diag > NEG // 2 else NEG
            g = max(g, e, F)
            rest = min(R - 1 - i, C - 1 - j)
            if g <= 0 or g + 5 * rest < S:
                g = NEG
            if e <= 0 or e + 5 * rest < S:
                e = NEG
            if g == S:
                return False
            diag = gp
            G[i], E[i] = g, e
            if g > NEG // 2 or e > NEG // 2:
                nlo = i if nlo < 0 else nlo
                nhi = i
            F = max(F - FT_GAP_EXT, g - FT_GAP_OPEN)
            if F <= 0:
                F = NEG
            if i > hi and F <= NEG // 2 and diag <= NEG // 2:
                break
            if i - lo + 2 >= ring:
                return True
            i += 1
        if nlo < 0:
            return False
        lo, hi = nlo, nhi
    return False


def finish_tier_restated(q, w, ends, bands, runs=0):
    """Which pass of run_finish must answer window w of query q, from the oracle's (score, ref_begin, ref_end, query_begin,
    query_end), the band widths its banded_sw went through and the number of runs of its CIGAR: 0 nothing aligned, 1 ... 4 the
    tier, 5 the replay.  A pass holds an alignment when
      LDS passes: the reverse pass fits the ring (not run for scores 148 ... 250, whose begin the exact reverse pass supplies), and
          for every band b: 2 * b + 3 + 1 <= band array entries and (2 * b + 1) * readLen <= direction cells;
      global passes: wcap = min(refLen + 3, FT_WCAP), the band arrays take 12 * wcap bytes of the slot and the direction rows the
          rest; for every band: 2 * b + 3 <= wcap or refLen + 3 <= FT_WCAP, and stride * readLen <= rest, where the stride is
          2 * b + 1, or refLen once 2 * b + 1 > refLen (dense rows, indexed by the column itself)."""
    s, rb, re_, qb, qe = ends
    if s <= 0:
        return 0
    if runs > FT_MAX_RUNS:
        return 5
    ref_len, read_len = re_ - rb + 1, qe - qb + 1
    assert bands and bands[0] == abs(ref_len - read_len) + 1
    need_rev = not 148 <= s < 251

    def lds(ring, arr, cells):
        if not all(2 * b + 3 + 1 <= arr and (2 * b + 1) * read_len <= cells for b in bands):
            return False
        return not (need_rev and _ft_ring_overflows(q, w, s, re_, qe, ring))

    def glob(slot, wcap_max):
        wcap = min(ref_len + 3, wcap_max)
        rest = slot - 12 * wcap
        if rest <= 0:
            return False
        for b in bands:
            stride = ref_len if 2 * b + 1 > ref_len else 2 * b + 1
            if (2 * b + 3 > wcap and ref_len + 3 > wcap_max) or stride * read_len > rest:
                return False
        return True

    if lds(FT_RING_1, FT_BAND_ARRAY_1, FT_CELLS_1):
        return 1
    if lds(FT_RING_2, FT_BAND_ARRAY_2, FT_CELLS_2):
        return 2
    if glob(FT_SLOT_3, FT_WCAP_3):
        return 3
    if glob(FT_SLOT_4, FT_WCAP_4):
        return 4
    return 5


def finish_tier_query(m):
    """The query of the finish-tier tests: seeded random ACGT of m rows with three low-complexity tracts of 72 rows, (GA)n, (GAA)n
    and a random homopurine run, from row m // 3 on, 150 rows apart (finish_tier_tracts)."""
    import synth
    q = bytearray(synth.random_rna(m, 8800000 + m))
    rng = synth._Rng(8810000 + m)
    for (lo, hi), unit in zip(finish_tier_tracts(m), (b"GA", b"GAA", None)):
        q[lo:hi] = bytes(unit[i % len(unit)] if unit else b"AG"[rng.below(2)] for i in range(hi - lo))
    return bytes(q)


def finish_tier_tracts(m):
    return tuple((m // 3 + 150 * k, m // 3 + 150 * k + 72) for k in range(3))


def _ft_shadow_rows(script):
    """Rows, relative to the first row of a planted alignment, that an F of 132 or more can reach below the planted path during
    the 8-bit forward pass: a path cell of H >= 148 in row r opens F = H - 16 in row r + 1, which loses 4 per row.  The pass ends
    at the first column whose maximum reaches 251, so nothing after that column counts."""
    rows, r, h = set(), -1, 0
    for op, n in script:
        for _ in range(n if op in "MX" else 1):
            if op == "M":
                r, h = r + 1, h + 5
            elif op == "X":
                r, h = r + 1, max(0, h - 4)
            else:
                h = max(0, h - FT_GAP_OPEN - FT_GAP_EXT * (n - 1))
                r += n if op == "I" else 0
            if h >= 148:
                rows.update(range(r + 1, r + 2 + (h - 148) // 4))
            if h >= 251:
                return rows
    return rows


def forward_pass_flags(q, w, r0=0, r1=None):
    """Does the systolic 8-bit forward pass flag window w (FwdOut.flags & 1 by its coarse test, the one queries with stripes of
    fewer than 96 rows get)?  It does when an F of 132 or more enters the first row of a stripe of the reference (rows k * ceil(m /
    16), k >= 1) in a column up to the first one whose maximum reaches 251, where the byte pass ends.  Plain Gotoh recurrences,
    a column at a time over query rows [r0, r1); F[i] = max over k < i of H[k] - 16 - 4 (i - k - 1) as a running maximum."""
    import numpy as np
    m = len(q)
    seg = (m + 15) // 16
    r1 = m if r1 is None else min(m, r1)
    r0 = max(0, r0)
    n = r1 - r0
    qa = np.frombuffer(q, dtype=np.uint8)[r0:r1]
    idx4 = 4 * np.arange(n, dtype=np.int64)
    starts = np.array([i for i in range(n) if (r0 + i) % seg == 0 and r0 + i > 0], dtype=np.int64)
    hp, ep = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for t in w:
        e = np.maximum(np.maximum(ep - FT_GAP_EXT, hp - FT_GAP_OPEN), 0)
        d = np.concatenate(([0], hp[:-1])) + np.where((qa == t) & (t in b"ACGT"), 5, -4)
        h0 = np.maximum(np.maximum(d, e), 0)
        run = np.maximum.accumulate(h0 + idx4)                      # max over k <= i of H[k] + 4 k
        f = np.concatenate(([0], run[:-1] - idx4[1:] - (FT_GAP_OPEN - FT_GAP_EXT)))      # F entering row i
        f = np.maximum(f, 0)
        if len(starts) and f[starts].max() >= 132:
            return True
        hp, ep = np.maximum(h0, f), e
        if hp.max() >= 251:
            return False
    return False


def planted_path_is_the_only_best(q, w, path, planted, r0=0, r1=None):
    """Is the planted path the one best local alignment of window w against query rows [r0, r1)?  path: column -> query row of the
    planted matches; planted: its score.  The recurrences of forward_pass_flags through every column, with all scores times 1 000
    and one more for a match that is not on the planted path: a path that reaches the planted score, or beats it, with the help of
    such a match (a flank that runs on into the bases next to it by chance, a cheaper way round a gap) ends above 1 000 * planted."""
    import numpy as np
    r1 = len(q) if r1 is None else min(len(q), r1)
    r0 = max(0, r0)
    n = r1 - r0
    qa = np.frombuffer(q, dtype=np.uint8)[r0:r1]
    idx4 = 4000 * np.arange(n, dtype=np.int64)
    hp, ep, best = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 0
    for c, t in enumerate(w):
        sc = np.where((qa == t) & (t in b"ACGT"), 5001, -4000)
        if c in path and 0 <= path[c] - r0 < n and sc[path[c] - r0] > 0:
            sc[path[c] - r0] = 5000
        e = np.maximum(np.maximum(ep - 1000 * FT_GAP_EXT, hp - 1000 * FT_GAP_OPEN), 0)
        h0 = np.maximum(np.maximum(np.concatenate(([0], hp[:-1])) + sc, e), 0)
        run = np.maximum.accumulate(h0 + idx4)
        f = np.maximum(np.concatenate(([0], run[:-1] - idx4[1:] - 1000 * (FT_GAP_OPEN - FT_GAP_EXT))), 0)
        hp, ep = np.maximum(h0, f), e
        best = max(best, int(hp.max()))
    return best == 1000 * planted


def finish_tier_windows(m, seed, with_scripts=False, query=None):
    """[(group, window)] (with_scripts: [(group, window, script)], None for a window without one) for the query finish_tier_query(m): windows of at most 200 nt, each a query slice with planted edits and
    0 ... 10 random bases on either side.  Edit scripts are lists of (op, n): 'M' n query rows copied, 'X' one row replaced by
    another base, 'I' n query rows left out (a run of I in the CIGAR), 'D' n random columns put in (a run of D).
    Groups: ungapped, one-gap, doubling, edges, ties, many-runs (see test_finish_tiers_cpu.py).  A 'D' gap of 100 columns is not
    in the set: either flank must score more than the gap costs, 5 f > 12 + 4 * 100, and two flanks of 83 do not fit 200 columns.
    Placement: the systolic 8-bit forward pass flags a window in which an F of 132 or more enters a stripe of the reference
    (every ceil(m / 16) rows), and a flagged window is replayed whatever its alignment needs.  The slice is therefore moved until
    no stripe boundary lies in the rows such an F can reach below the planted path (_ft_shadow_rows), and the window is kept only
    if the forward recurrences themselves show no such F (forward_pass_flags: the diagonal that runs on past the end of a flank
    stays above 148 for as long as chance has it); otherwise the slice moves on.  The finish kernels then get every window.
    A window is also kept only if the planted path is its one best alignment (planted_path_is_the_only_best), so that the oracle's
    CIGAR shows the planted gaps; the bases around the slice and at the ends of an inserted run are picked not to continue a flank.
    A script for which 48 slices fail either test is left out (test_finish_tiers_cpu.py names the one that the set may lack).
    Slices keep 300 rows clear of the tracts, which at 1 200 rows leaves the starts 10 ... 24 (plus up to a stripe) and 787 ... 824:
    about half of the windows there begin within 100 rows of the query's start, where the reverse pass runs out of query before it
    runs out of ring, so ring overflow at 1 200 rows is exercised by the other half and by the 3 300-row query."""
    import synth
    rng = synth._Rng(seed)
    q = finish_tier_query(m) if query is None else query          # (another query of m rows: its ties group holds no tracts)
    assert len(q) == m
    seg = (m + 15) // 16
    tracts = finish_tier_tracts(m)
    free = [(10, tracts[0][0] - 300 - seg), (tracts[2][1] + 15, m - 300 - seg)]   # slice starts that keep 300 rows clear of the tracts
    out = []

    def rnd(n, first_not=None, last_not=None):
        s = bytearray(b"ACGT"[rng.below(4)] for _ in range(n))
        if n and first_not is not None:
            s[0] = next(c for c in b"ACGT"[rng.below(4):] + b"ACGT" if c != first_not)
        if n and last_not is not None and (n > 1 or first_not is None or s[-1] == last_not):
            s[-1] = next(c for c in b"ACGT"[rng.below(4):] + b"ACGT" if c != last_not and (n > 1 or c != first_not))
        return bytes(s)

    def row(i):
        return q[i] if 0 <= i < m else None

    def build(script, a, left, right):
        """the window of `script` applied to the query from row a on, with `left` / `right` random bases around it: an inserted or
        added base never matches the query row that the alignment would reach next, so the planted ends and gaps stay put"""
        w, i, path = bytearray(), a, {}
        for op, n in script:
            if op == "M":
                path.update((left + len(w) + d, i + d) for d in range(n))
                w += q[i:i + n]
                i += n
            elif op == "X":
                w += rnd(1, first_not=q[i])
                i += 1
            elif op == "I":
                i += n
            else:
                ins = bytearray(rnd(n, first_not=row(i), last_not=row(i - 1)))
                # eight bases at either end that do not continue the flank next to them, straight on or after a gap of one
                for d in range(min(8, n // 2)):
                    ins[d] = next(c for c in b"ACGT" if c not in (row(i + d - 1), row(i + d), row(i + d + 1)))
                    ins[n - 1 - d] = next(c for c in b"ACGT" if c not in (row(i - 2 - d), row(i - 1 - d), row(i - d)))
                w += ins
        assert i <= m
        # the bases around the slice: random, but none continues the alignment straight on or after a gap of one
        lpad, rpad = bytearray(rnd(left)), bytearray(rnd(right))
        for d in range(left):
            lpad[left - 1 - d] = next(c for c in b"ACGT"[rng.below(4):] + b"ACGT" if c not in (row(a - 2 - d), row(a - 1 - d), row(a - d)))
        for d in range(right):
            rpad[d] = next(c for c in b"ACGT"[rng.below(4):] + b"ACGT" if c not in (row(i + d - 1), row(i + d), row(i + d + 1)))
        return bytes(lpad) + bytes(w) + bytes(rpad), path

    def place(script, a=None):
        rows = sum(n for op, n in script if op in "MI") + sum(1 for op, _ in script if op == "X")
        shadow = _ft_shadow_rows(script)
        if a is None:
            lo, hi = free[rng.below(2)]
            a = lo + rng.below(hi - lo)
            a = next((a + d for d in range(seg + 1) if not any((a + d + r) % seg == 0 for r in shadow)), None)
            if a is None:                # the rows such an F reaches cover a whole stripe: this script cannot avoid the flag
                return None
        assert a + rows <= m and not any((a + r) % seg == 0 and a + r < m for r in shadow), (script, a)
        return a

    def add(group, script, a=None, left=None, right=None):
        fixed = a is not None
        rows = sum(n for op, n in script if op in "MI") + sum(1 for op, _ in script if op == "X")
        cols = sum(n for op, n in script if op in "MD") + sum(1 for op, _ in script if op == "X")
        left = rng.below(11) if left is None else left
        right = rng.below(11) if right is None else right
        left, right = min(left, (FT_MAX_WINDOW - cols) // 2), min(right, (FT_MAX_WINDOW - cols + 1) // 2)
        planted = sum(5 * n if op == "M" else -4 if op == "X" else -(FT_GAP_OPEN + FT_GAP_EXT * (n - 1)) for op, n in script)
        a = place(script, a)
        for _ in range(48):
            if a is None:
                return                   # no placement of this script escapes the flag
            w, path = build(script, a, left, right)
            assert 0 < len(w) <= FT_MAX_WINDOW, (group, script)
            # kept if the byte pass does not flag it and nothing beats the planted path (a flank that runs on into the bases next
            # to it by chance, a cheaper way round a gap); the tracts have their ties and a gap of one residue often has two places to
            # be, so those two groups are kept as they come
            if not forward_pass_flags(q, w, a - 12, a + rows + 80) and (group in ("ties", "many-runs") or planted_path_is_the_only_best(q, w, path, planted, a - 12, a + rows + 12)):
                out.append((group, w, script))
                return
            a = a if fixed else place(script)          # (a fixed slice is tried again with other bases around it)

    def spread(n, nx):
        """n rows with nx of them replaced, evenly"""
        if not nx:
            return [("M", n)]
        head = []
        if n > 60:                       # (the first 52 rows stay whole: the byte pass is over before the first replaced row)
            head, n = [("M", 52)], n - 52
        nx = min(nx, n // 3)             # (at most every second row of what is left)
        step, s = n // (nx + 1), head
        assert step >= 2, (n, nx)
        for _ in range(nx):
            s += [("M", step - 1), ("X", 1)]
        return s + [("M", n - nx * step)]

    # ungapped: below 148 (up to 29 rows), 148 ... 250 (30 ... 50 rows), 251 and more; the replaced rows lower the score below
    # 5 per column, which is what lets the reverse pass keep many rows alive (and leave the 64-row ring)
    for n in (20, 24, 27, 29, 30, 33, 40, 45, 50, 51, 60, 64, 65, 66, 80, 100, 128, 150, 190):
        add("ungapped", [("M", n)])
    for n, nx in ((40, 6), (44, 7), (60, 4), (60, 11), (64, 12), (80, 6), (80, 15), (100, 8), (100, 20), (128, 12), (150, 14), (150, 30), (190, 10), (190, 20), (190, 40)):
        add("ungapped", spread(n, nx))
    # 251 and more that stay in the 64-row ring: the F chain below a cell of value g lives for (g - 16) / 4 rows of the reverse pass,
    # pruned or not, and walks out of the ring unless the query ends first, so these start less than 60 rows into the query
    for i, n in enumerate((55, 60, 70, 80, 90, 100, 110, 120, 52, 57, 65, 75)):
        add("ungapped", [("M", n)], a=46 + i if m < 3072 else 5 + 4 * i)
    # one gap: the shortest flanks that still make the joined alignment beat either flank, and long flanks
    for k in FT_ONE_GAP:
        for op in "ID":
            room = 190 if op == "I" else 198 - k             # (a long gap leaves little for the random bases around the slice)
            if 2 * ((12 + 4 * k) // 5 + 1) > room:
                assert (op, k) == ("D", 100)
                continue
            fmin = min((12 + 4 * k) // 5 + 9, room // 2)         # 40 above the gap's cost: more than a flank gains by running on by chance
            for f in sorted({fmin, min(room // 2, max(fmin + 12, 32)), min(90, room // 2)}):
                add("one-gap", [("M", f), (op, k), ("M", f)])
    # below 148 with a band of 15 ... 17: out of the 16 KB LDS pass by the band array alone
    for f1, op, k, f2 in ((18, "I", 14, 18), (19, "I", 15, 19), (20, "D", 14, 20), (18, "D", 15, 19), (20, "I", 16, 20), (21, "D", 16, 21), (19, "D", 14, 18), (20, "I", 15, 21)):
        add("one-gap", [("M", f1), (op, k), ("M", f2)])
    # a 'D' gap of 62 or 63 columns between flanks of 54 ... 58: band 63 or 64 is too wide for the 64 KB LDS pass (2 b + 4 > 128)
    # while (2 b + 1) * readLen still fits the 16 KB slot next to its band arrays, which sends the window to the 16 KB global pass
    for k, f1, f2 in [(62, f1, f2) for f1 in range(54, 59) for f2 in range(54, 59) if f1 + f2 <= 112] + [(63, f1, f2) for f1 in range(54, 57) for f2 in range(54, 57) if f1 + f2 <= 110]:
        add("one-gap", [("M", f1), ("D", k), ("M", f2)])
    # doubling: refLen == readLen, the band starts at 1 and doubles until it holds both gaps
    # Each outer flank pays for the gap next to it with 40 to spare.  The middle flank has to outweigh BOTH gaps (24 + 8 k) against the
    # path that stays near the diagonal through the f + k unrelated columns between the outer flanks, which chance makes cheaper than
    # 1.75 a column: it gets what 200 columns leave, up to 70 rows.  Up to k = 9 also three short flanks (below 251).
    for k in FT_DOUBLING:
        fmin = max(20, (12 + 4 * k) // 5 + 9)
        for ops in ("ID", "DI"):
            for f, mid in sorted({(fmin, fmin) if k <= 9 else (fmin, min(70, 190 - k - 2 * fmin)), (fmin, min(70, 190 - k - 2 * fmin))}):
                add("doubling", [("M", f), (ops[0], k), ("M", mid), (ops[1], k), ("M", f)])
    # edges
    add("edges", [("M", 28)], a=0)
    add("edges", [("M", 34)], a=0, left=0)
    add("edges", [("M", 20), ("D", 3), ("M", 22)], left=0)
    add("edges", [("M", 26)], a=m - 26)
    add("edges", [("M", 60)], a=m - 60, right=0)
    add("edges", [("M", 22), ("I", 2), ("M", 24)], right=0)
    add("edges", [("M", 70)], left=0, right=0)
    out.append(("edges", q[m // 2:m // 2 + 1], None))            # one column
    out.append(("edges", FT_NO_MATCH, None))                     # no match at all
    # ties: slices of the low-complexity tracts with small indels, below 148 (no F of 132 anywhere, so any rows will do)
    for t, (lo, hi) in enumerate(tracts):
        for j, (f1, op, k, f2) in enumerate(((12, "I", 1, 12), (10, "D", 1, 14), (13, "I", 2, 13), (12, "D", 2, 13), (14, "I", 3, 12), (11, "D", 3, 14),
                                              (27, "M", 0, 0), (9, "D", 1, 9))):
            script = [("M", f1)] + ([(op, k), ("M", f2)] if k else [])
            add("ties", script, a=lo + 3 + 5 * j + t)
    # many runs: 7-row blocks separated by 1-residue gaps of one kind, every gap pays (35 > 16): 51, 49, 53 and 51 runs
    for pattern, blocks in (("I", 26), ("D", 25), ("I", 27), ("I", 26)):
        script = [("M", 7)]
        for g in range(blocks - 1):
            script += [(pattern[g % len(pattern)], 1), ("M", 7)]
        add("many-runs", script)
    return out if with_scripts else [(g, w) for g, w, _ in out]


_FT_CENSUS = {}


def finish_tier_census(orc, m):
    """The windows of query length m with the oracle's answer and the restated tier, computed once and shared: dicts group, window,
    script, ends (score, ref_begin, ref_end, query_begin, query_end), cigar, tainted, bands, runs, cls, tier."""
    if m not in _FT_CENSUS:
        q, rows = finish_tier_query(m), []
        for g, w, script in finish_tier_windows(m, FT_SEED + m, with_scripts=True):
            ends, cig, tainted, bands = orc.align_ex(q, w)
            runs = sum(c in "MID" for c in cig)
            rows.append({"group": g, "window": w, "script": script, "ends": ends, "cigar": cig, "tainted": tainted, "bands": bands, "runs": runs,
                         "cls": score_class(ends[0]), "tier": finish_tier_restated(q, w, ends, bands, runs)})
        _FT_CENSUS[m] = (q, rows)
    return _FT_CENSUS[m]


FT_SCAN_M = 1200
FT_SCAN_ENCS = (22, 23, 26, 27, 40, 41)      # one-to-one encodings: every query letter has a pre-image


def finish_tier_scan_case(orc):
    """(query, 10 kb DNA record of two segments, plants) for the scan-level finish test: random DNA with the pre-images of 24 gapped
    windows planted in it, all below 251 (a scan never finishes an alignment of 251 or more): first those with a band too wide for the
    16 KB LDS pass (restated tier 2), those without inserted columns before the others.  The query is random without two equal letters in a
    row: under the one-to-one encodings a repeated query letter is a TT or CC of the strand a triplex record shows, which costs the
    record 1 000 of stability (penaltyT, penaltyC), and no record would come of the plants.  Two plants of neighbouring scores
    share a unit, so that neither falls below the unit's threshold of 0.8 times its best stage-1 score.
    plants: dicts seg, enc, pos, n, qb, qe (query rows), cigar."""
    import synth
    rng = synth._Rng(8820000)
    q = bytearray(b"A")
    while len(q) < FT_SCAN_M:
        q.append([c for c in b"ACGT" if c != q[-1]][rng.below(3)])
    q = bytes(q)
    rows = []
    for g, w, script in finish_tier_windows(FT_SCAN_M, FT_SEED + 7, with_scripts=True, query=q):
        if g not in ("one-gap", "doubling"):
            continue
        ends, cig, tainted, bands = orc.align_ex(q, w)
        if score_class(ends[0]) != "hi" and not tainted:
            rows.append({"window": w, "ends": ends, "cigar": cig, "inserted": any(op == "D" for op, _ in script),
                         "tier": finish_tier_restated(q, w, ends, bands, sum(c in "MID" for c in cig))})
    rows.sort(key=lambda r: (r["tier"] != 2, r["inserted"], -r["ends"][0]))
    picked = sorted(rows[:24], key=lambda r: r["ends"][0])
    assert len(picked) == 24, len(rows)
    dna = bytearray(synth.random_dna(10000, 8830000))
    plants = []
    for i, r in enumerate(picked):
        unit, slot = i // 2, i % 2
        s, enc = unit // 6, FT_SCAN_ENCS[unit % 6]
        tract = preimage(r["window"], enc, rng)
        pos = 4900 * s + 300 + 2100 * slot + 150 * (unit % 6)
        dna[pos:pos + len(tract)] = tract
        plants.append({"seg": s, "enc": enc, "pos": pos, "n": len(tract), "qb": r["ends"][3], "qe": r["ends"][4], "cigar": r["cigar"]})
    assert len(dna) == 10000
    return q, bytes(dna), plants


def finish_tier_oracle_scan(build_dir, tmp_dir, q, dna):
    """the oracle's `scan` of the scan-level case (cLength 20 = ntMin), parsed: (meta, units)"""
    import synth
    rna_fa, dna_fa = os.path.join(str(tmp_dir), "ftq.fa"), os.path.join(str(tmp_dir), "ftd.fa")
    synth.write_fasta(rna_fa, "ftq", q)
    synth.write_fasta(dna_fa, f"syn|chrT|1-{len(dna)}", dna)
    return parse_scan(oracle_cli(build_dir, "scan", rna_fa, dna_fa, "-threads", "8"))


def finish_tier_planted_records(units, plants):
    """plants whose unit holds a triplex record over at least 30 of the plant's query rows"""
    hit = []
    for p in plants:
        for u in units:
            if (u["seg"], u["enc"]) != (p["seg"], p["enc"]):
                continue
            for x in u["triplexes"]:
                a, b = sorted((int(x[0]), int(x[1])))
                if min(b - 1, p["qe"]) - max(a - 1, p["qb"]) + 1 >= 30:
                    hit.append(p)
                    break
    return hit


# ---- classic SIM (-F) at strip, chunk and node-list edges (test_sim_edges_cpu.py, test_gpu_sim_edges.py) ------------------------
# Triplex targets are purine tracts: repeats and homopolymers give many cells of one score and many nodes tied for the lowest score,
# which is where addnode()'s "first node of lowest score gives way" and the prefix maxima of the re-sweeps can go wrong unnoticed.
SIM_K = 50
SIM_EDGE_HEADER = "syn|chrE|1-%d"


def _sim_edge_stretches(n, rng):
    """n letters in stretches of 8 ... 40 nt: random ACGT, a GA repeat, a homopolymer or a TC repeat (either phase)"""
    out = bytearray()
    while len(out) < n:
        ln, kind = 8 + rng.below(33), rng.below(4)
        if kind == 0:
            out += bytes(b"ACGT"[rng.below(4)] for _ in range(ln))
        elif kind == 2:
            out += bytes([b"AGTC"[rng.below(4)]]) * ln
        else:
            ph = rng.below(2)
            out += ((b"GA" if kind == 1 else b"TC") * 21)[ph:ph + ln]
    return out[:n]


def sim_edge_query(m, seed):
    """A query of m rows, upper-case ACGT, in stretches of random letters, GA repeats, homopolymers and TC repeats."""
    import synth
    return bytes(_sim_edge_stretches(m, synth._Rng(seed * 2654435761 + 11)))


def sim_edge_dna(n, seed):
    """DNA of n letters built like sim_edge_query, with an N every 40 ... 99 letters (none in a record shorter than that)."""
    import synth
    rng = synth._Rng(seed * 40503 + 29)
    dna = _sim_edge_stretches(n, rng)
    i = 40 + rng.below(60)
    while i < n:
        dna[i] = ord("N")
        i += 40 + rng.below(60)
    return bytes(dna)


# -- (a) the forward sweep called directly: queries x targets x compositions x thresholds
SIM_FWD_M = (1, 2, 63, 64, 65, 127, 128, 129, 200)          # zero, one or two full strips of 64 rows, last_lane 0 and 63
SIM_FWD_N = (1, 2, 63, 64, 65, 127, 128, 129, 257)          # shorter than a 64-column prefetch chunk, and ending at 64 k +- 1
SIM_FWD_COMPOSITIONS = ("random", "AG", "homopolymer", "GA/AG", "withN")
SIM_FWD_THRESHOLDS = ("0", "50", "140", "near-best", "100000")
SIM_FWD_BATCHES = (1, 5, 7)                                 # targets per call, in turn: not multiples of the 4 units of a workgroup


def sim_forward_inputs(comp, m):
    """(query of m rows, one target per length of SIM_FWD_N) of a composition.  The targets are what k_sim_forward compares with the
    query letter by letter (no rule encoding in between)."""
    import synth
    k = SIM_FWD_COMPOSITIONS.index(comp)
    seed = 7000 + 100 * k + m

    def two_letter(n, s, ab):
        return bytes(ab[c in b"AC"] for c in synth.random_dna(n, s))

    if comp == "random":
        return synth.random_rna(m, seed), [synth.random_dna(n, seed + 1000 + n) for n in SIM_FWD_N]
    if comp == "AG":
        return two_letter(m, seed, b"AG"), [two_letter(n, seed + 1000 + n, b"AG") for n in SIM_FWD_N]
    if comp == "homopolymer":
        return b"A" * m, [b"A" * n for n in SIM_FWD_N]
    if comp == "GA/AG":
        return (b"GA" * m)[:m], [(b"AG" * n)[:n] for n in SIM_FWD_N]
    return sim_edge_query(m, seed), [sim_edge_dna(n, seed + n) for n in SIM_FWD_N]


def sim_forward_problems(orc, comp, m):
    """(query, [(target, threshold name, min_score)]) of one query: every target at every threshold of SIM_FWD_THRESHOLDS, the
    lengths in turn, so that a batch holds targets of different lengths.  `near-best` is 60 below the best x10 score of the pair (the
    largest node score at threshold 0; the best node never gives way, being the lowest only when all 50 are equal): the cells within
    one match of the best, a handful."""
    q, targets = sim_forward_inputs(comp, m)
    out = []
    for name in SIM_FWD_THRESHOLDS:
        for t in targets:
            if name == "near-best":
                best = max([x[0] for x in orc.sim_forward_nodes(q, t, 0)], default=0)
                thr = max(0, best - 60)
            else:
                thr = int(name)
            out.append((t, name, thr))
    return q, out


def sim_forward_batches(problems):
    """the problems of one query cut into calls of 1, 5, 7, 1, 5, 7 ... targets"""
    out, i, k = [], 0, 0
    while i < len(problems):
        n = SIM_FWD_BATCHES[k % len(SIM_FWD_BATCHES)]
        out.append(problems[i:i + n])
        i, k = i + n, k + 1
    return out


def sim_list_state(nodes):
    return "empty" if not nodes else "full" if len(nodes) == SIM_K else "partial"


def sim_tied_lowest(nodes):
    """nodes of a FULL list that share its lowest score (1: no tie); 0 for a list that is not full"""
    if len(nodes) < SIM_K:
        return 0
    low = min(x[0] for x in nodes)
    return sum(x[0] == low for x in nodes)


def sim_row_events_at_least(q, t):
    """A lower bound of the largest number of cells of one row above a threshold below 50: a cell whose letters match scores 50 or more."""
    return max(sum(c == a and c in b"ACGT" for c in t) for a in set(q))


# -- (b) ... (e) whole scans.  A numbered table of named cases: id -> (query rows, query seed, record lengths, first record seed)
SIM_SCAN_M = (63, 64, 65, 128, 129, 200)
SIM_SCAN_N = (63, 65, 129, 300)
SIM_EDGE_CASES = {}
for _i, _m in enumerate(SIM_SCAN_M):
    for _j, _n in enumerate(SIM_SCAN_N):
        SIM_EDGE_CASES[f"b{4 * _i + _j:02d}-m{_m}-n{_n}"] = (_m, 300 + _m, (_n,), 500 + 10 * _m + _n)
SIM_EDGE_CASES["b09-m65-n65"] = (65, 365, (65,), 1217)        # (the record of seed 1215 leaves nothing above the tail filter)
SIM_SUSPEND_CASES =("b00-m63-n63", "b05-m64-n65", "b10-m65-n129", "b12-m128-n63")          # (c)
SIM_EDGE_CASES["d-m64-8rec"] = (64, 364, (63, 300, 97, 211, 65, 158, 129, 263), 900)       # (d) 8 records x 48 units in one batch
# (e) lists that stay partial; the seeds are ones whose record is not a single repeated letter (such a segment is skipped)
for _k, (_m, _n, _s) in enumerate(((20, 6, 907), (20, 10, 915), (20, 16, 919), (65, 6, 1357), (65, 10, 1362))):
    SIM_EDGE_CASES[f"e{_k}-m{_m}-n{_n}"] = (_m, 300 + _m, (_n,), _s)
SIM_PARTIAL_CASES = tuple(k for k in SIM_EDGE_CASES if k.startswith("e"))


def sim_edge_case(name):
    """(query, [record, ...]) of a case of SIM_EDGE_CASES"""
    m, qseed, lens, dseed = SIM_EDGE_CASES[name]
    return sim_edge_query(m, qseed), [sim_edge_dna(n, dseed + r) for r, n in enumerate(lens)]


def simscan_units(text):
    """`simscan` lines -> per unit, in file order, {'seg', 'enc', 'n', 'thr', 'x': the 13-field X tuples as scan() gives them}"""
    units = []
    for line in text.decode().splitlines():
        f = line.split(" ")
        if f[0] == "V":
            units.append({"seg": int(f[1]), "enc": int(f[2]), "n": int(f[7]), "thr": int(f[9]), "x": []})
        elif f[0] == "X":
            units[-1]["x"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]),
                                   int(f[10], 16), int(f[11], 16), f[12].encode(), f[13].encode()))
    return units


def simscan_triplexes(text, c_length, min_identity=60.0, min_stability=1.0):
    """X lines of `simscan` with LongTarget()'s tail filter (Fasim-LongTarget.cpp:589-597; SIM() itself only filters on nt), as
    scan() tuples"""
    import struct
    out = []
    for u in simscan_units(text):
        for x in u["x"]:
            ident = struct.unpack("<f", struct.pack("<I", x[9]))[0]
            tri = struct.unpack("<f", struct.pack("<I", x[10]))[0]
            if float(x[8]) >= 0.0 and ident >= min_identity and tri >= min_stability and x[7] >= c_length:
                out.append(x + (u["seg"], u["enc"]))
    return out


_SIM_EDGE_SIMSCAN = {}


def sim_edge_simscan(build_dir, tmp_dir, q, dna, c_length=10):
    """the oracle's `simscan -lg c_length` of one record (made once per query and record, and left unchanged)"""
    import synth
    key = (q, dna, c_length)
    if key not in _SIM_EDGE_SIMSCAN:
        rna_fa, dna_fa = os.path.join(str(tmp_dir), "simq.fa"), os.path.join(str(tmp_dir), "simd.fa")
        synth.write_fasta(rna_fa, "simq", q)
        synth.write_fasta(dna_fa, SIM_EDGE_HEADER % len(dna), dna)
        _SIM_EDGE_SIMSCAN[key] = oracle_cli(build_dir, "simscan", rna_fa, dna_fa, "-lg", str(c_length), "-threads", "8")
    return _SIM_EDGE_SIMSCAN[key]


def sim_edge_census(orc, build_dir, tmp_dir, name, c_length=10):
    """Per record of a case: the units' forward-sweep lists by state, the X records of the oracle and those left by the tail filter.
    [{'units', 'empty', 'partial', 'full', 'two_nodes', 'tied': full lists with two or more nodes of the lowest score, 'sweeps': units
    whose first round ends in a re-sweep, 'partial_sweeps': those of them with a partial list, 'x', 'kept'}]"""
    q, recs = sim_edge_case(name)
    rows = []
    for dna in recs:
        text = sim_edge_simscan(build_dir, tmp_dir, q, dna, c_length)
        units = simscan_units(text)
        row = {"units": len(units), "empty": 0, "partial": 0, "full": 0, "two_nodes": 0, "tied": 0, "sweeps": 0, "partial_sweeps": 0,
               "x": sum(len(u["x"]) for u in units), "kept": len(simscan_triplexes(text, c_length))}
        for u in units:
            t, _ = orc.encode_unit(dna, u["enc"])
            nodes = orc.sim_forward_nodes(q, t, u["thr"])
            row[sim_list_state(nodes)] += 1
            row["two_nodes"] += len(nodes) >= 2
            row["tied"] += sim_tied_lowest(nodes) >= 2
            # the first round ends in a re-sweep when its node passes the threshold and is not the only one (sim.h:594, 884)
            sweeps = len(nodes) >= 2 and max(x[0] for x in nodes) / 10.0 > u["thr"]
            row["sweeps"] += sweeps
            row["partial_sweeps"] += sweeps and len(nodes) < SIM_K
        rows.append(row)
    return rows


# ---- the triplex scan off its default parameters (test_scan_params_cpu.py, test_gpu_scan_params.py) -----------------------------
# With the defaults penaltyT = -1000 takes 1 000 of stability from every alignment that shows two T in a row, and minStability = 1,
# minIdentity = 60 and ntMin = 20 then drop it: most of what stage 3 computes never becomes a record.  "Open" filters keep them all.
SCAN_OPEN = ("-pt", "0", "-pc", "0", "-S", "-100000", "-i", "0", "-ni", "1")
SCAN_Q2_SEGMENTS = 12          # open_q2 scans the first 12 of q2cat.fa's 19 segments: the whole file's scan is too large to commit
# name -> (query, DNA file, options of `scan`, which are the reference CLI's); ref_probe `scan -detail 0` of each is
# tests/golden/params_<name>.scan.gz (`make_golden.py params`)
SCAN_PARAM_PINNED = {
    "open": ("H19", "planted40k.fa", SCAN_OPEN),
    "open_meg3": ("MEG3", "planted40k.fa", SCAN_OPEN),
    "open_demo": ("H19", "testDNA.fa", SCAN_OPEN),
    "open_q2": ("H19", "q2cat.fa", SCAN_OPEN + ("-o", "0")),
    "pen": ("H19", "planted40k.fa", ("-pt", "-3", "-pc", "-2", "-S", "-50")),
    # -S -50 drops nothing (a mean stability is never below the penalties), so in `pen` the penalties only show in the records'
    # stability; with -S 1 they also decide which alignments become records.  The engine filters twice, on the numbers-only
    # conversion before it builds a record's strings and on the record itself: only a stability that the first conversion puts
    # too low loses a record, so each penalty is once the milder of the two
    "pen_stab": ("H19", "planted40k.fa", ("-pt", "-3", "-pc", "-2", "-S", "1", "-i", "0", "-ni", "1")),
    "pen_stab_swapped": ("H19", "planted40k.fa", ("-pt", "-2", "-pc", "-3", "-S", "1", "-i", "0", "-ni", "1")),
    "ntmax": ("H19", "planted40k.fa", ("-na", "40", "-ni", "30")),
    "thresholds": ("H19", "planted40k.fa", ("-i", "70", "-S", "2")),
    "cut5001": ("H19", "planted40k.fa", SCAN_OPEN + ("-c", "5001", "-o", "100")),
    "cut12345": ("H19", "planted40k.fa", SCAN_OPEN + ("-c", "12345", "-o", "2000")),
    "cut20000": ("H19", "planted40k.fa", SCAN_OPEN + ("-c", "20000", "-o", "0")),
    "cut40000": ("H19", "planted40k.fa", SCAN_OPEN + ("-c", "40000", "-o", "100")),
}
SCAN_THRESHOLD_CASES = ("thresholds",)
SCAN_CUT_CASES = ("cut5001", "cut12345", "cut20000", "cut40000")
# the two smallest cut lengths take their expectation from the live oracle (3 312 and 480 units)
SCAN_PARAM_LIVE_CUTS = {
    "cut64": ("MEG3", "testDNA.fa", SCAN_OPEN + ("-c", "64", "-o", "0")),
    "cut777": ("H19", "testDNA.fa", SCAN_OPEN + ("-c", "777", "-o", "333")),
}
# (rule, strand) -> number of encodings enabled
SCAN_RULE_STRAND = {(6, 1): 2, (7, 0): 2, (18, -1): 2, (1, -1): 2, (3, 0): 4}
SCAN_NO_ENCODINGS = ((7, 1), (19, 0))
_SCAN_OPTION_FIELDS = {"-r": "rule", "-t": "strand", "-c": "cutLength", "-o": "overlapLength", "-i": "minIdentity", "-S": "minStability",
                       "-ni": "ntMin", "-na": "ntMax", "-pc": "penaltyC", "-pt": "penaltyT", "-ds": "cDistance", "-lg": "cLength"}


def scan_option_fields(options):
    """Options of the reference CLI as fields of the parameter structure: {'penaltyT': 0, ...}."""
    assert len(options) % 2 == 0
    return {_SCAN_OPTION_FIELDS[k]: int(v) for k, v in zip(options[::2], options[1::2])}


def scan_param_dna(golden_dir, name, dna_file):
    """(header, DNA) of a case: the fixture's record, for open_q2 its first SCAN_Q2_SEGMENTS whole segments."""
    import synth
    hdr, dna = synth.read_fasta(os.path.join(golden_dir, dna_file))
    if name == "open_q2":
        dna = dna[:SCAN_Q2_SEGMENTS * 5000]
        hdr = "syn|chrQ|1-%d" % len(dna)
    return hdr, dna


def scan_param_files(golden_dir, tmp_dir, name, case):
    """(query path, DNA path) of a case for the oracle's command line; a shortened record is written under tmp_dir."""
    import synth
    query, dna_file, _ = case
    dna_fa = os.path.join(golden_dir, dna_file)
    if name == "open_q2":
        hdr, dna = scan_param_dna(golden_dir, name, dna_file)
        dna_fa = os.path.join(str(tmp_dir), "q2cat_%d.fa" % SCAN_Q2_SEGMENTS)
        synth.write_fasta(dna_fa, hdr, dna)
    return os.path.join(golden_dir, query + ".fa"), dna_fa


_SCAN_PARAM_FIXTURES = {}


def scan_param_fixture(golden_dir, name):
    """(meta, units) of tests/golden/params_<name>.scan.gz, parsed once and left unchanged."""
    if name not in _SCAN_PARAM_FIXTURES:
        _SCAN_PARAM_FIXTURES[name] = parse_scan(gunzip(os.path.join(golden_dir, f"params_{name}.scan.gz")))
    return _SCAN_PARAM_FIXTURES[name]


# ---- the banded stage 3 at class, zone and bound edges (test_band_edges_cpu.py, test_gpu_band_edges.py) --------------------------
# The smallest query lengths at which each band class, zone count and tile count of band.hip first occurs (1 008: no band yet;
# 6 000: the tile boundary, row 3 000, is not the zone boundary, row 3 072).
BAND_EDGE_LENGTHS = (1008, 1009, 2017, 3073, 4081, 6000)
# segments [0, 5 000) and [4 900, 9 900) at the default 5 000 / 100, and the short tail segment [9 800, 9 900) of 100 columns
BAND_EDGE_DNA_LEN = 9900
BAND_EDGE_SEGMENTS = ((0, 5000), (4900, 5000), (9800, 100))
BAND_EDGE_ENCS = (22, 23, 26, 27, 40, 41)       # one-to-one encodings, as in the row-layout sweep: a plant reads in one unit only
BAND_EDGE_LOW_ENCS = (26, 40, 41)                # their units hold the plants of 120 to 130, the others those of 135 to 145
BAND_EDGE_FLANK = 40                            # N on either side of every plant
BAND_EDGE_JOINT = 12                            # N between a candidate and the neighbour that ends just after its window
BAND_EDGE_HOT_ENC = 22                          # the first segment's unit of this encoding holds the 160-point plant and two of 145
# twins (name, first row of the upper copy, distance to the lower copy, rows, which copy is one match longer).  Every copy starts
# at a row = 14 (mod 48), so that none contains a whole 24-row plant around a multiple of 48.  With a window of about 110 columns a
# path of 130 may span 212 rows, so twins 96 rows apart still fit 384 rows, 432 apart only 768, 1 008 apart only 1 536.
BAND_EDGE_TWINS = (("twin-96", 62, 96, 26, None), ("twin-432", 302, 432, 26, None), ("twin-1008", 398, 1008, 26, None),
                   ("twin-1728", 446, 1728, 26, None), ("near-twin-upper", 110, 96, 26, "upper"), ("near-twin-lower", 254, 96, 26, "lower"))
# tall plants: skipped query rows g -> rows of the two exact parts, as long as keeps 5 (a + b) - 12 - 4 g below 148 (141 ... 145)
BAND_EDGE_TALL = {1: (16, 16), 4: (17, 17), 8: (18, 19), 12: (20, 21), 16: (22, 22)}
BAND_EDGE_WIDE = (1, 4, 8)                      # the mirror image: g extra DNA letters between the parts
BAND_EDGE_TALL_EDGES = (10, 11, 12, 13, 17, 18, 19, 20)    # multiples of 48 (rows 480 ... 960) that the tall and wide plants cross


def band_layout_restated(m):
    """(profile lanes nl, zone stride, zones, classes G) of the banded stage 3 for a query of m rows: band_profile_lanes,
    band_zone_stride and band_classes of band.hip written out (not imported from the library), with the 72 KB LDS condition and the
    14-bit stream-word condition."""
    seg = (m + 15) // 16
    nl = (16 * seg + 47) // 48
    zs = 64
    while (nl + zs - 1) // zs > 32:
        zs *= 2
    zs = min(zs, nl)
    classes = []
    if seg >= 8 and (seg + 191) // 192 <= 31:
        for G in (8, 16, 32):
            lc = min(zs + G, nl)
            lds = (5 * lc + G) * 112 + 8 * 64 * 16
            if 8 * G <= 3 * nl and lds <= 72 * 1024 and (5 * lc + G) * 7 < 0x4000:
                classes.append(G)
    return nl, zs, (nl + zs - 1) // zs, classes


def scan_lane_of_row(m, row):
    """Global virtual lane of k_scan that owns query row `row` (lane_rows of systolic.h, inverted)."""
    seg, vs, _ = systolic_layout(m)
    s, off = divmod(row, seg)
    q, rem = divmod(seg, vs)
    j = off // (q + 1) if off < rem * (q + 1) else rem + (off - rem * (q + 1)) // q
    return s * vs + j


def _band_edge_other(avoid):
    return next(c for c in b"ACGT" if c not in avoid)


def band_edge_inputs(m):
    """(query, DNA record, plants) of the band-edge sweep's case of m rows.

    Query: seeded random ACGT with the copies of BAND_EDGE_TWINS written in.  DNA: synth.random_dna of BAND_EDGE_DNA_LEN with exact
    and gapped pre-images of query rows under BAND_EDGE_ENCS, those of one unit at least 250 columns apart unless they are meant as
    neighbours.  Each lies between two runs of BAND_EDGE_FLANK N (-4 against every row in stages 2 and 3, -1 in stage 1): with a
    query of thousands of rows the background offers a piece of 17 or more beside almost any cell, and without the N every second
    plant grows by a gapped or mismatched extension; crossing forty N costs 160 in a window and 40 in stage 1, which sets the
    unit's threshold.  (Between a candidate and the neighbour that must end just after its window there are BAND_EDGE_JOINT.)  Every plant
    scores below 148 in its own window: 24 rows (120) as a rule, twins 26 or 27, the candidates beside the 160-point plant 27, the
    long neighbour 29.
    plants: dicts name, kind, enc, pos / n (DNA), rows [(lo, hi)] of the exact parts in path order, score and q_end (the row the
    deciding try must end at); gap = skipped query rows (tall), ins = extra DNA letters (wide), hot = the 160-point plant."""
    import synth
    nl, zs, zones, classes = band_layout_restated(m)
    seg = (m + 15) // 16
    rng = synth._Rng(8800000 + m)
    q = bytearray(synth.random_rna(m, 8100000 + m))
    twins = []
    for name, r, delta, rows, longer in BAND_EDGE_TWINS:
        if r + delta + rows + 2 > m:
            continue
        q[r + delta - 1:r + delta + rows + 1] = q[r - 1:r + rows + 1]
        if longer:       # the longer copy's extra row; the other copy must not have it
            q[(r if longer == "lower" else r + delta) + rows] = _band_edge_other({q[(r + delta if longer == "lower" else r) + rows]})
        twins.append((name, r, delta, rows, longer))
    q = bytes(q)
    dna = bytearray(synth.random_dna(BAND_EDGE_DNA_LEN, 8200000 + m))
    plants = []

    def put(name, kind, enc, pos, parts, ins=0, before=BAND_EDGE_FLANK, after=BAND_EDGE_FLANK, **extra):
        """writes the pre-image of the rows `parts` (ranges in path order) at DNA base `pos`, between runs of `before` and `after` N"""
        text = bytearray(q[parts[0][0]:parts[0][1]])
        for a, b in parts[1:]:
            # (wide) extra letters that match neither the row before nor the row after the break
            text += bytes(_band_edge_other({q[a - 1], q[a]}) for _ in range(ins))
            text += q[a:b]
        tract = preimage(bytes(text), enc, rng)
        n = len(tract)
        assert pos >= 0 and pos + n <= len(dna), (name, pos)
        lo, hi = max(0, pos - before), min(len(dna), pos + n + after)
        dna[lo:hi] = b"N" * (pos - lo) + tract + b"N" * (hi - pos - n)
        nrows = sum(b - a for a, b in parts)
        gap = parts[1][0] - parts[0][1] if len(parts) > 1 else 0
        score = 5 * nrows - (12 + 4 * max(gap, ins) if len(parts) > 1 else 0)
        p = {"name": name, "kind": kind, "enc": enc, "pos": pos, "n": n, "rows": list(parts), "score": score, "q_end": parts[-1][1] - 1}
        if ins:
            p["ins"] = ins
        p.update(extra)
        plants.append(p)
        return p

    # ---- the plants that go wherever there is room: units of the five other encodings in both long segments
    free = []
    def room(name, kind, parts, **kw):
        free.append((name, kind, parts, kw))

    room("top", "top", [(0, 24)])
    room("bottom", "bottom", [(m - 24, m)])
    ks = {16: "lane-edge-mid"}
    for G in classes:
        ks.setdefault(nl - G, f"lane-edge-last-start-G{G}")
        ks.setdefault(nl - G + 1, f"lane-edge-past-last-start-G{G}")
    for k, name in sorted(ks.items()):
        if 48 * k + 12 <= m:
            room(name, "lane-edge", [(48 * k - 12, 48 * k + 12)])
    if m >= 3073:
        for lo in (3060, 3048, 3072):
            if lo + 24 <= m:
                room(f"zone-edge-{lo}", "zone-edge", [(lo, lo + 24)])
        room("tile-edge", "tile-edge", [(8 * seg - 12, 8 * seg + 12)])
    for name, r, delta, rows, longer in twins:
        if longer == "lower":
            room(name, "twin", [(r + delta, r + delta + rows + 1)], upper=r, delta=delta)
        else:
            room(name, "twin", [(r, r + rows + (1 if longer else 0))], upper=r, delta=delta)
    edges = list(BAND_EDGE_TALL_EDGES)
    for g, (a, b) in sorted(BAND_EDGE_TALL.items()):
        e = 48 * edges.pop(0)
        lo = e - a - g // 2
        room(f"tall-{g}", "tall", [(lo, lo + a), (lo + a + g, lo + a + g + b)], gap=g, edge=e)
        if m >= 3072 + g + b + 1:
            lo = 3072 - a - g // 2
            room(f"tall-{g}-zone-edge", "tall", [(lo, lo + a), (lo + a + g, lo + a + g + b)], gap=g, edge=3072)
    for g in BAND_EDGE_WIDE:
        a, b = BAND_EDGE_TALL[g]
        e = 48 * edges.pop(0)
        room(f"wide-{g}", "wide", [(e - a, e), (e, e + b)], ins=g, edge=e)
    # Stage 1 scores N as -1, so a unit's maximum is its best plant plus up to about 15 of background from across the N, and a
    # candidate must beat 0.8 of that: plants of 120 to 130 share units (encodings BAND_EDGE_LOW_ENCS), plants of 135 to 145 share
    # the others.  Alternately in the two long segments, 150 bases apart, each class's encodings in turn: 300 columns or more
    # between plants of one unit.
    turn = {}
    for i, (name, kind, parts, kw) in enumerate(free):
        s, j = i % 2, i // 2
        low = 5 * sum(b - a for a, b in parts) <= 130
        encs = [enc for enc in BAND_EDGE_ENCS if (enc in BAND_EDGE_LOW_ENCS) == low and (s, enc) != (0, BAND_EDGE_HOT_ENC)]
        k = turn[(s, low)] = turn.get((s, low), -1) + 1
        put(name, kind, encs[k % len(encs)], BAND_EDGE_SEGMENTS[s][0] + 200 + 150 * j + (7 * i) % 13, parts, **kw)

    # ---- column edges (even encodings: a DNA base is its unit's column)
    put("first-columns", "column-edge", 26, 2, [(700, 724)])
    put("overlap", "column-edge", 40, 4930, [(710, 734)])
    put("tail-segment", "column-edge", 40, 9805, [(730, 754)])
    put("last-columns", "column-edge", 26, 9873, [(740, 764)])

    def block_pos(base, row):
        """the first column pe >= base with (pe + lane of `row` inside its tile) % 64 == 10: k_scan's step of that lane at column pe
        and at the 53 columns after it lie in one block of 64 steps"""
        v = scan_lane_of_row(m, row) % 128
        return base + (10 - (base + v)) % 64

    # ---- hot neighbour: a 29-row candidate and, after the run of N that ends it, 32 rows (160) far below: they end 44 columns
    #      after the candidate's window, in the same 64-step block of their last lane.  The same candidate rows again 600 columns on.
    #      (Two alignments of one unit cannot share columns, so a neighbour ends at least its own length after the window.)
    pe = block_pos(4000, 881)
    put("hot-neighbour-near", "hot-neighbour", BAND_EDGE_HOT_ENC, pe - 28, [(600, 629)], after=BAND_EDGE_JOINT)
    put("hot", "hot", BAND_EDGE_HOT_ENC, pe + 1 + BAND_EDGE_JOINT, [(850, 882)], before=0, hot=True)
    put("hot-neighbour-far", "hot-neighbour", BAND_EDGE_HOT_ENC, pe + 600, [(640, 669)])
    # ---- loose neighbour: A (27 rows) and, after the run of N that ends it, B (29 rows, 145) more than the tallest band below A:
    #      B ends 41 columns after A's window in the same block of its last lane
    if classes:
        d = 48 * classes[-1] + 60
        pe = BAND_EDGE_SEGMENTS[1][0] + block_pos(4700, 520 + d + 28)      # (in the second segment's unit)
        put("loose-A", "loose-neighbour", 22, pe - 26, [(520, 547)], after=BAND_EDGE_JOINT)
        put("loose-B", "loose-neighbour", 22, pe + 1 + BAND_EDGE_JOINT, [(520 + d, 520 + d + 29)], before=0)
    assert len(dna) == BAND_EDGE_DNA_LEN
    return q, bytes(dna), plants


def band_edge_unit_columns(p):
    """[(segment, last column of the plant in that segment's unit of its encoding)] for the segments that hold the whole plant"""
    out = []
    for s, (start, n) in enumerate(BAND_EDGE_SEGMENTS):
        if start <= p["pos"] and p["pos"] + p["n"] <= start + n:
            first = p["pos"] - start
            out.append((s, n - 1 - first if p["enc"] & 1 else first + p["n"] - 1))
    return out


def band_edge_files(tmp_dir, m):
    """Writes the case of m rows as two FASTA files under tmp_dir: (query path, DNA path, query, DNA, plants)."""
    import synth
    rna, dna, plants = band_edge_inputs(m)
    rna_fa, dna_fa = os.path.join(str(tmp_dir), f"bandq{m}.fa"), os.path.join(str(tmp_dir), f"bandd{m}.fa")
    synth.write_fasta(rna_fa, f"bandq{m}", rna)
    synth.write_fasta(dna_fa, f"syn|chrB|1-{len(dna)}", dna)
    return rna_fa, dna_fa, rna, dna, plants


def band_edge_oracle_scan(build_dir, tmp_dir, m, detail=1, threads=8):
    """The oracle's `scan` of the case with open filters (SCAN_OPEN): raw text."""
    rna_fa, dna_fa, _, _, _ = band_edge_files(tmp_dir, m)
    return oracle_cli(build_dir, "scan", rna_fa, dna_fa, "-detail", str(detail), "-threads", str(threads), *SCAN_OPEN)
