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
