"""Sites above a fixed potential (fasim_scan_records_sites), the part that needs no GPU: the yardstick of the GPU tests -- the site
list of DESIGN.md section 14 from the restatement's potential P and its per-encoding maxima (test_track_cpu.py; it never calls the
code under test), checked here against a brute-force loop over positions -- and the two pure host functions of the C-ABI,
fasim_sites_merge and fasim_sites_bed."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from test_track_cpu import colmax_units, enabled_encodings, enc_class, encode_unit, same_seq


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def expected_potential(rna, dna, p, seg_first=0, seg_count=-1):
    """P[c][x] of sections 11 / 14 for one record as a (4, n) array, and per enabled encoding the maximum over the selected units
    that cover x of the unit's value at x (-1 where none does): what expected() of test_gpu_screen.py builds, both halves kept."""
    big = len(dna)
    step = p.cutLength - p.overlapLength
    starts = list(range(0, big, step))
    last = len(starts) if seg_count < 0 else min(len(starts), seg_first + seg_count)
    encs = enabled_encodings(p)
    out = np.zeros((4, big), dtype=np.int64)
    per_enc = {e: np.full(big, -1, dtype=np.int64) for e in encs}
    for a in starts[max(0, seg_first):last]:
        seg = dna[a:a + p.cutLength]
        if same_seq(seg):
            continue
        cm = colmax_units(rna, [encode_unit(seg, e) for e in encs])
        for k, e in enumerate(encs):
            row = cm[k][::-1] if e & 1 else cm[k]
            c = enc_class(e)
            out[c, a:a + len(seg)] = np.maximum(out[c, a:a + len(seg)], row)
            per_enc[e][a:a + len(seg)] = np.maximum(per_enc[e][a:a + len(seg)], row)
    return out, per_enc


def raw_runs(row, v):
    """[(a, b)] of the maximal ranges with row[x] >= v, vectorised."""
    on = np.concatenate(([0], (np.asarray(row) >= v).astype(np.int8), [0]))
    d = np.diff(on)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def sites_from(P, per_enc, v, gap=0):
    """The site list of the definition as an (n, 6) int64 array of (cls, start, end, value, pos, enc), ordered by (start, cls).
    per_enc: {encoding: (n,) array}, the class of an encoding from enc_class()."""
    rows = []
    for c in range(4):
        chain = []
        for a, b in raw_runs(P[c], v):
            if chain and a - chain[-1][1] <= gap:
                chain[-1][1] = b
            else:
                chain.append([a, b])
        for a, b in chain:
            value = int(P[c, a:b].max())
            pos = a + int(np.argmax(P[c, a:b]))
            enc = min(e for e, arr in per_enc.items() if enc_class(e) == c and arr[pos] == value)
            rows.append((c, a, b, value, pos, enc))
    rows.sort(key=lambda r: (r[1], r[0]))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 6)


def sites_brute(P, per_enc, v, gap):
    """The same by one loop over the positions of every class: a site stays open until a position more than `gap` past its last
    position of value >= v is reached."""
    rows = []
    n = P.shape[1]
    for c in range(4):
        start = end = None
        for x in range(n + gap + 2):
            if start is not None and x > end + gap:
                best, pos = -1, -1
                for y in range(start, end):
                    if P[c, y] > best:
                        best, pos = int(P[c, y]), y
                enc = next(e for e in sorted(per_enc) if enc_class(e) == c and per_enc[e][pos] == best)
                rows.append((c, start, end, best, pos, enc))
                start = end = None
            if x < n and P[c, x] >= v:
                if start is None:
                    start = x
                end = x + 1
    rows.sort(key=lambda r: (r[1], r[0]))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 6)


def _random_potential(rng, n, encs):
    per_enc = {e: rng.integers(0, 9, size=n).astype(np.int64) for e in encs}
    for arr in per_enc.values():
        arr[rng.random(n) < 0.5] = 0
    P = np.zeros((4, n), dtype=np.int64)
    for e, arr in per_enc.items():
        P[enc_class(e)] = np.maximum(P[enc_class(e)], arr)
    return P, per_enc


@pytest.mark.parametrize("gap", [0, 1, 5])
def test_helper_equals_the_brute_force_loop(gap):
    rng = np.random.default_rng(100 + gap)
    encs = [0, 1, 2, 3, 12, 13, 14, 15, 16]
    seen = 0
    for trial in range(30):
        n = int(rng.integers(1, 60))
        P, per_enc = _random_potential(rng, n, encs)
        for v in (1, 3, 6, 9):
            got, want = sites_from(P, per_enc, v, gap), sites_brute(P, per_enc, v, gap)
            assert np.array_equal(got, want), (trial, v, got.tolist(), want.tolist())
            seen += len(got)
            for c, a, b, value, pos, enc in got.tolist():
                assert 0 <= a < b <= n and P[c, a] >= v and P[c, b - 1] >= v and value == P[c, a:b].max() >= v and a <= pos < b
    assert seen > 200


@pytest.mark.parametrize("gap", [0, 3])
def test_sites_merge_of_two_overlapping_shards_is_the_unsplit_list(mod, gap):
    """A random potential cut in two with an overlap: each shard's list is the definition on its own positions, the merged list the
    definition on all of them."""
    rng = np.random.default_rng(7 + gap)
    encs = [0, 1, 2, 3, 12, 13, 14, 15]
    for trial in range(20):
        n = int(rng.integers(20, 120))
        P, per_enc = _random_potential(rng, n, encs)
        cut, overlap = int(rng.integers(1, n - 8)), int(rng.integers(0, 8))
        v = int(rng.integers(1, 7))
        shards = []
        for k, (lo, hi) in enumerate(((0, cut + overlap), (cut, n))):
            Pk = np.zeros_like(P)
            Pk[:, lo:hi] = P[:, lo:hi]
            pk = {e: np.where((np.arange(n) >= lo) & (np.arange(n) < hi), arr, -1) for e, arr in per_enc.items()}
            shards.append(mod.Sites(sites_from(Pk, pk, v, gap), min_value=v, max_gap=gap, units=10 + k, saturated_units=k, raw_runs=5 + k))
        got = mod.merge_sites(shards)
        want = sites_from(P, per_enc, v, gap)
        assert got.array().dtype == np.int64 and np.array_equal(got.array(), want), (trial, got.array().tolist(), want.tolist())
        assert (got.units, got.saturated_units, got.raw_runs, got.min_value, got.max_gap, len(got)) == (21, 1, 11, v, gap, len(want))


def test_sites_merge_tie_rules_and_refusals(mod):
    S = mod.Sites
    # abutting intervals join at gap 0; larger value wins, then the smaller pos, then the smaller enc; classes never join
    a = S([(0, 10, 20, 50, 12, 14), (1, 10, 20, 50, 12, 14), (2, 0, 5, 9, 1, 12)], min_value=5)
    b = S([(0, 20, 30, 50, 25, 0), (1, 21, 30, 60, 25, 1), (2, 3, 8, 9, 1, 3)], min_value=5)
    c = S([(0, 15, 18, 50, 12, 2)], min_value=5)
    got = mod.merge_sites([a, b, c]).array().tolist()
    assert got == [[2, 0, 8, 9, 1, 3], [0, 10, 30, 50, 12, 2], [1, 10, 20, 50, 12, 14], [1, 21, 30, 60, 25, 1]]
    # the same lists at gap 1: the two class-1 intervals join and the larger value carries its own pos and enc
    a1, b1 = (S(x.array(), min_value=5, max_gap=1) for x in (a, b))
    assert mod.merge_sites([a1, b1]).array().tolist() == [[2, 0, 8, 9, 1, 3], [0, 10, 30, 50, 12, 14], [1, 10, 30, 60, 25, 1]]
    one = mod.merge_sites([a])
    assert np.array_equal(one.array(), a.array()[np.lexsort((a.array()[:, 0], a.array()[:, 1]))])
    assert mod.merge_sites([S(None, min_value=5), S(None, min_value=5)]).array().shape == (0, 6)
    for other in (S(b.array(), min_value=6), S(b.array(), min_value=5, max_gap=1)):
        with pytest.raises(mod.FasimError) as ei:
            mod.merge_sites([a, other])
        assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_sites([])
    assert ei.value.code == mod.E_ARG


def test_sites_bed_bytes(mod):
    """0-based half-open genome coordinates (start_genome = 1-based position of the record's first base), + for ParaPlus / AntiPlus and
    - for the Minus classes, the Rule column of -TFOsorted (encodings 0-11: enc // 2 + 1, 12-47: (enc - 12) // 2 + 1)."""
    t = mod.Sites([(0, 0, 7, 61, 3, 4), (1, 5, 9, 80, 8, 11), (2, 5, 6, 70, 5, 46), (3, 100, 140, 16383, 139, 13)], min_value=60, max_gap=5)
    head = "# fasim sites lncRNA=MEG3 min_value=60 max_gap=5\n"
    body8 = ("chr14\t1000\t1007\tParaPlus\t61\t+\t1003\t3\n"
             "chr14\t1005\t1009\tParaMinus\t80\t-\t1008\t6\n"
             "chr14\t1005\t1006\tAntiMinus\t70\t-\t1005\t18\n"
             "chr14\t1100\t1140\tAntiPlus\t16383\t+\t1139\t1\n")
    assert mod.sites_bed(t, "chr14", 1001, "MEG3") == (head + body8).encode()
    assert mod.sites_bed(t, "chr14", 1001, "MEG3", header=False) == body8.encode()
    # start_genome 1: genome coordinate == record position
    want9 = ("c\t0\t7\tParaPlus\t61\t+\t3\t3\tpeak_7\nc\t5\t9\tParaMinus\t80\t-\t8\t6\tpeak_7\n"
             "c\t5\t6\tAntiMinus\t70\t-\t5\t18\tpeak_7\nc\t100\t140\tAntiPlus\t16383\t+\t139\t1\tpeak_7\n")
    assert mod.sites_bed(t, "c", 1, "MEG3", record_name="peak_7", header=False) == want9.encode()
    assert mod.sites_bed(t, "c", 1, "q", record_name="peak_7") == ("# fasim sites lncRNA=q min_value=60 max_gap=5\n" + want9).encode()
    empty = mod.Sites(None, min_value=1)
    assert mod.sites_bed(empty, "c", 1, "q") == b"# fasim sites lncRNA=q min_value=1 max_gap=0\n"
    assert mod.sites_bed(empty, "c", 1, "q", header=False) == b""
    with pytest.raises(mod.FasimError) as ei:
        mod.sites_bed(mod.Sites([(4, 0, 1, 5, 0, 0)], min_value=1), "c", 1, "q")
    assert ei.value.code == mod.E_ARG


def test_sites_objects_round_trip(mod):
    rows = np.array([[3, 2 ** 33, 2 ** 33 + 4, 16383, 2 ** 33 + 1, 47], [0, 5, 6, 1, 5, 0]], dtype=np.int64)
    t = mod.Sites(rows, min_value=1, max_gap=2, units=96, saturated_units=1, raw_runs=9)
    assert np.array_equal(t.array(), rows)
    assert (t.n, t.units, t.saturated_units, t.raw_runs, t.min_value, t.max_gap) == (2, 96, 1, 9, 1, 2)


def test_sites_symbols_are_exported(mod):
    for s in ("fasim_scan_records_sites", "fasim_sites_merge", "fasim_sites_bed", "fasim_sites_free"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
    assert hasattr(mod.Engine, "scan_sites")


@pytest.mark.parametrize("gap", [0, 1, 5])
def test_runs_cut_at_slice_and_segment_edges_unite_to_the_definition(mod, gap):
    """What the engine does with the kernel's output, on a small scale: overlapping segments (length 50, step 40) with their own
    values, every segment cut into slices of 17 positions, the runs of every (segment, slice, class) with their own value, pos and
    enc.  United by the library's sweep (fasim_sites_merge of one list) they are the sites of P = the maximum over the segments."""
    rng = np.random.default_rng(40 + gap)
    encs = [0, 1, 2, 3, 12, 13, 14, 15]
    for trial in range(25):
        n = int(rng.integers(30, 200))
        v = int(rng.integers(1, 7))
        P = np.zeros((4, n), dtype=np.int64)
        per_enc = {e: np.full(n, -1, dtype=np.int64) for e in encs}
        rows = []
        for a in range(0, n, 40):
            b = min(n, a + 50)
            Ps, ps = _random_potential(rng, b - a, encs)
            if trial % 3 == 0:
                Ps, ps = np.minimum(Ps + 5, 8), {e: np.minimum(x + 5, 8) for e, x in ps.items()}      # long runs across every edge
            P[:, a:b] = np.maximum(P[:, a:b], Ps)
            for e in encs:
                per_enc[e][a:b] = np.maximum(per_enc[e][a:b], ps[e])
            for s0 in range(0, b - a, 17):
                s1 = min(b - a, s0 + 17)
                cut = sites_from(Ps[:, s0:s1], {e: x[s0:s1] for e, x in ps.items()}, v, 0)
                cut[:, [1, 2, 4]] += a + s0
                rows.append(cut)
        rows = np.concatenate(rows)
        rng.shuffle(rows)
        got = mod.merge_sites([mod.Sites(rows, min_value=v, max_gap=gap)])
        want = sites_from(P, per_enc, v, gap)
        assert np.array_equal(got.array(), want), (trial, got.array().tolist(), want.tolist())


@pytest.mark.parametrize("args", [["--sites", "100x"], ["--sites", ""], ["--sites", "99999999999999999999"], ["--sites", "4294967356"],
                                  ["--sites", "60", "--sites-gap", "5y"], ["--sites", "60", "--sites-gap", "4294967297"]])
def test_cli_refuses_numbers_with_trailing_characters_or_out_of_range(tmp_path, args):
    """--sites and --sites-gap take whole decimal integers: `100x` is not 100 and 2^32 + 60 is not 60.  Status 2 before any
    device is opened, nothing written."""
    import subprocess
    exe = os.path.join(entry.PKG_DIR, "fasim")
    gold = os.path.join(entry.ROOT, "tests", "golden")
    r = subprocess.run([exe, "-f1", os.path.join(gold, "testDNA.fa"), "-f2", os.path.join(gold, "H19.fa"), "-O", str(tmp_path) + "/"] + args,
                       capture_output=True)
    assert r.returncode == 2, r.stderr
    assert os.listdir(tmp_path) == []
