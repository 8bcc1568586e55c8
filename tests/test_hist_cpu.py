"""Histograms of the potential with shuffled controls, the part that needs no GPU: the pure host functions of
the C-ABI -- fasim_shuffle_query, fasim_hist_merge, fasim_hist_threshold, fasim_hist_tsv -- against restatements of their
definitions written here, which never call the code under test."""
import itertools
import os

import numpy as np
import pytest

import __graft_entry__ as entry

BINS = 16384
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


# ---- the shuffle ---------------------------------------------------------------------------------------------------------------------
def shuffle_restated(rna: bytes, seed: int, k: int) -> bytes:
    s = (seed ^ (k * 0xD1B54A32D192ED03)) & MASK
    a = bytearray(rna)
    for i in range(len(a) - 1, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & MASK
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        j = z % (i + 1)
        a[i], a[j] = a[j], a[i]
    return bytes(a)


@pytest.mark.parametrize("m", [1, 2, 113, 2812])
def test_shuffle_equals_the_restated_generator(mod, m):
    rng = np.random.default_rng(m)
    rna = bytes(rng.choice(np.frombuffer(b"ACGUTacgun", dtype=np.uint8), size=m).tobytes())
    for seed, k in ((0, 1), (0, 2), (7, 1), (7, 3), (2 ** 64 - 1, 1), (0x123456789ABCDEF0, 40000)):
        got = mod.shuffle_query(rna, seed, k)
        assert got == shuffle_restated(rna, seed, k), (seed, k)
        assert sorted(got) == sorted(rna)
    if m >= 113:
        assert mod.shuffle_query(rna, 7, 1) != mod.shuffle_query(rna, 7, 2) != rna
        assert mod.shuffle_query(rna, 7, 1) != mod.shuffle_query(rna, 8, 1)
    for bad in ((b"", 0, 1), (b"ACGT", 0, 0)):
        with pytest.raises(mod.FasimError) as ei:
            mod.shuffle_query(*bad)
        assert ei.value.code == mod.E_ARG


# ---- the merge -----------------------------------------------------------------------------------------------------------------------
CUT, OVL = 10, 3
STEP = CUT - OVL


def _toy_records():
    """Two records of 4 and 2 segments (cut 10, overlap 3), per segment a (4, len) array of its own values; segment 2 of record 0 is
    'skipped' (zeros), so boundaries 1 and 2 of record 0 pair a side with a same-letter neighbour."""
    rng = np.random.default_rng(17)
    recs = []
    for n in (27, 12):
        segs = []
        for a in range(0, n, STEP):
            ln = min(CUT, n - a)
            segs.append(rng.integers(0, 40, size=(4, ln)).astype(np.uint16))
        recs.append((n, segs))
    recs[0][1][2][:] = 0
    return recs


def _toy_hist(mod, recs, first, count):
    """The histogram of global segments [first, first + count) by the definition: covered positions with the maximum over the
    selected segments, and a pending edge for every boundary with exactly one side selected."""
    counts = np.zeros((4, BINS), dtype=np.int64)
    pending, g, units = [], 0, 0
    for r, (n, segs) in enumerate(recs):
        P = np.zeros((4, n), dtype=np.int64)
        cov = np.zeros(n, dtype=bool)
        sel = [first <= g + i < first + count for i in range(len(segs))]
        for i, v in enumerate(segs):
            if sel[i]:
                a = i * STEP
                P[:, a:a + v.shape[1]] = np.maximum(P[:, a:a + v.shape[1]], v)
                cov[a:a + v.shape[1]] = True
                units += 1
        for b in range(len(segs) - 1):
            if sel[b] != sel[b + 1]:
                ln = segs[b + 1][:, :OVL].shape[1]
                pending.append((r, b, 0, segs[b][:, STEP:STEP + ln]) if sel[b] else (r, b, 1, segs[b + 1][:, :ln]))
        for c in range(4):
            counts[c] += np.bincount(P[c][cov], minlength=BINS)
        g += len(segs)
    return mod.Hist(counts, units=units, saturated_units=count, pending=pending)


def _key(h):
    return (h.array().tolist(), h.positions, h.units, h.saturated_units, [(r, b, s, v.tolist()) for r, b, s, v in h.pending])


def test_merge_pairs_the_pending_edges(mod):
    recs = _toy_records()
    nseg = sum(len(s) for _, s in recs)
    assert nseg == 6
    whole = _toy_hist(mod, recs, 0, nseg)
    assert whole.positions == 27 + 12 and not whole.pending and all(int(whole.array()[c].sum()) == 39 for c in range(4))
    # the construction is not vacuous: some overlap position differs between its two segments, so the shards' counts do not just add
    one = [_toy_hist(mod, recs, s, 1) for s in range(nseg)]
    assert sum(h.array() for h in one).tolist() != whole.array().tolist()
    assert [len(h.pending) for h in one] == [1, 2, 2, 1, 1, 1]
    # two parts, cut at every boundary (within a record, beside the skipped segment, between the records), both orders
    for k in range(1, nseg):
        a, b = _toy_hist(mod, recs, 0, k), _toy_hist(mod, recs, k, nseg - k)
        assert len(a.pending) == len(b.pending) == (0 if k == 4 else 1)
        for parts in ((a, b), (b, a)):
            assert _key(mod.merge_hists(parts)) == _key(whole), k
    # three parts, every order and nesting; partial merges keep exactly the edges of the union
    for i, j in itertools.combinations(range(1, nseg), 2):
        parts = [_toy_hist(mod, recs, 0, i), _toy_hist(mod, recs, i, j - i), _toy_hist(mod, recs, j, nseg - j)]
        for perm in itertools.permutations(range(3)):
            x, y, z = (parts[t] for t in perm)
            assert _key(mod.merge_hists([x, y, z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_hists([mod.merge_hists([x, y]), z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_hists([x, mod.merge_hists([y, z])])) == _key(whole), (i, j, perm)
        assert _key(mod.merge_hists(parts[:2])) == _key(_toy_hist(mod, recs, 0, j))
        assert _key(mod.merge_hists(parts[1:])) == _key(_toy_hist(mod, recs, i, nseg - i))
        outer = mod.merge_hists([parts[0], parts[2]])            # not neighbours: nothing pairs
        assert outer.positions == parts[0].positions + parts[2].positions
        assert len(outer.pending) == len(parts[0].pending) + len(parts[2].pending)
    # all six single segments
    assert _key(mod.merge_hists(one)) == _key(whole) and _key(mod.merge_hists(one[::-1])) == _key(whole)
    assert _key(mod.merge_hists([whole])) == _key(whole)


def test_merge_refusals(mod):
    recs = _toy_records()
    a = _toy_hist(mod, recs, 0, 2)
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_hists([a, a])                                    # the same edge pending twice: the parts overlap
    assert ei.value.code == mod.E_ARG
    z = np.zeros((4, BINS), dtype=np.int64)
    x = mod.Hist(z, pending=[(0, 1, 0, np.zeros((4, 3)))])
    y = mod.Hist(z, pending=[(0, 1, 1, np.zeros((4, 2)))])
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_hists([x, y])
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_hists([])
    assert ei.value.code == mod.E_ARG


# ---- the threshold -------------------------------------------------------------------------------------------------------------------
def _hist_of(mod, values):
    """values: {class: {value: count}}"""
    a = np.zeros((4, BINS), dtype=np.int64)
    for c, d in values.items():
        for v, n in d.items():
            a[c, v] = n
    return mod.Hist(a)


def threshold_restated(real, controls, Q):
    K = len(controls)
    ge = real.array().sum(axis=0)[::-1].cumsum()[::-1]
    cge = sum((c.array().sum(axis=0) for c in controls), np.zeros(BINS, dtype=np.int64))[::-1].cumsum()[::-1]
    for v in range(1, BINS):
        if ge[v] > 0 and all(float(cge[w]) <= Q * float(K) * float(ge[w]) for w in range(v, BINS) if ge[w] > 0):
            return v
    return 0


def test_threshold_on_hand_made_curves(mod):
    # a non-monotone fdr: fine at 5 and 6, too many control hits at 8, fine again from 9 on
    real = _hist_of(mod, {0: {0: 1000, 5: 100, 6: 50, 8: 10, 9: 10, 30: 5}, 3: {0: 1165, 9: 10}})
    ctl = [_hist_of(mod, {0: {0: 1170, 5: 2, 8: 3}, 1: {0: 1175}}), _hist_of(mod, {2: {0: 1171, 8: 4}})]
    assert threshold_restated(real, ctl, 0.05) == 9 and mod.hist_threshold(real, ctl, 0.05) == 9
    assert mod.hist_threshold(real, ctl, 1.0) == threshold_restated(real, ctl, 1.0) == 1
    for q in (0.001, 0.02, 0.1, 0.14, 0.15, 0.5):
        assert mod.hist_threshold(real, ctl, q) == threshold_restated(real, ctl, q), q
    # K = 0: no control can object; the smallest value is 1 wherever anything is above 0
    assert mod.hist_threshold(real, [], 0.05) == threshold_restated(real, [], 0.05) == 1
    # holes: ge is flat between the values that occur, the answer may fall into a hole
    holes = _hist_of(mod, {1: {0: 50, 40: 3, 100: 2}})
    hctl = [_hist_of(mod, {1: {0: 54, 40: 1}})]
    assert mod.hist_threshold(holes, hctl, 0.05) == threshold_restated(holes, hctl, 0.05) == 41
    # nothing below Q: the controls reach the top value as often as the query
    same = [_hist_of(mod, {0: {0: 1000, 5: 100, 6: 50, 8: 10, 9: 10, 30: 5}, 3: {0: 1165, 9: 10}})]
    assert mod.hist_threshold(real, same, 0.05) == threshold_restated(real, same, 0.05) == 0
    # nothing above 0 at all
    flat = _hist_of(mod, {c: {0: 10} for c in range(4)})
    assert mod.hist_threshold(flat, [], 0.05) == 0 and mod.hist_threshold(flat, [flat], 0.05) == 0
    # a control above the query's top does not count: no w >= v has ge[w] > 0 there
    high = [_hist_of(mod, {0: {0: 1, 200: 7}})]
    assert mod.hist_threshold(holes, high, 0.05) == threshold_restated(holes, high, 0.05)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(mod.FasimError) as ei:
            mod.hist_threshold(real, ctl, bad)
        assert ei.value.code == mod.E_ARG


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_tsv_bytes(mod):
    real = _hist_of(mod, {0: {0: 96, 2: 3, 4: 1}, 1: {0: 100}, 2: {0: 99, 1: 1}, 3: {0: 98, 4: 2}})
    head = "value\tParaPlus\tParaPlus_ge\tParaMinus\tParaMinus_ge\tAntiMinus\tAntiMinus_ge\tAntiPlus\tAntiPlus_ge\tall_ge\n"
    want = ("# fasim potential histogram lncRNA=MEG3 positions=100\n" + head +
            "1\t0\t4\t0\t0\t1\t1\t0\t2\t7\n2\t3\t4\t0\t0\t0\t0\t0\t2\t6\n3\t0\t1\t0\t0\t0\t0\t0\t2\t3\n4\t1\t1\t0\t0\t0\t0\t2\t2\t3\n")
    assert mod.hist_tsv(real, "MEG3") == want.encode()
    ctl = [_hist_of(mod, {0: {0: 99, 1: 1}, 1: {0: 100}, 2: {0: 100}, 3: {0: 100}}),
           _hist_of(mod, {0: {0: 100}, 1: {0: 99, 6: 1}, 2: {0: 100}, 3: {0: 100}})]
    headc = ("value\tParaPlus\tParaPlus_ge\tParaPlus_ctl_ge\tParaMinus\tParaMinus_ge\tParaMinus_ctl_ge\tAntiMinus\tAntiMinus_ge\t"
             "AntiMinus_ctl_ge\tAntiPlus\tAntiPlus_ge\tAntiPlus_ctl_ge\tall_ge\tall_ctl_ge\tfdr\n")
    wantc = ("# fasim potential histogram lncRNA=MEG3 positions=100 controls=2 seed=7 fdr=0.1 min_value=NA\n" + headc +
             "1\t0\t4\t1\t0\t0\t1\t1\t1\t0\t0\t2\t0\t7\t2\t0.142857\n"
             "2\t3\t4\t0\t0\t0\t1\t0\t0\t0\t0\t2\t0\t6\t1\t0.0833333\n"
             "3\t0\t1\t0\t0\t0\t1\t0\t0\t0\t0\t2\t0\t3\t1\t0.166667\n"
             "4\t1\t1\t0\t0\t0\t1\t0\t0\t0\t2\t2\t0\t3\t1\t0.166667\n"
             "5\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\t1\tNA\n"
             "6\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\t1\tNA\n")
    assert mod.hist_tsv(real, "MEG3", ctl, seed=7, fdr=0.1) == wantc.encode()         # (at 4: 1 control hit > 0.1 * 2 * 3)
    assert mod.hist_tsv(real, "MEG3", ctl, seed=7, fdr=0.25) == wantc.replace("fdr=0.1 min_value=NA", "fdr=0.25 min_value=1").encode()
    # with a threshold: only control 0, whose single hit at value 1 is within 0.25 of the query's 7
    got = mod.hist_tsv(real, "q", ctl[:1], seed=2 ** 64 - 1, fdr=0.25).decode().splitlines()
    assert got[0] == "# fasim potential histogram lncRNA=q positions=100 controls=1 seed=18446744073709551615 fdr=0.25 min_value=1"
    assert len(got) == 2 + 4 and got[2].split("\t")[-3:] == ["7", "1", "0.142857"]
    empty = _hist_of(mod, {c: {0: 5} for c in range(4)})
    assert mod.hist_tsv(empty, "q") == ("# fasim potential histogram lncRNA=q positions=5\n" + head).encode()


def test_hist_object_and_symbols(mod):
    a = np.zeros((4, BINS), dtype=np.int64)
    a[:, 0] = 7
    a[2, 16383] = 2
    a[2, 0] = 5
    h = mod.Hist(a, units=3, saturated_units=1)
    assert h.array().dtype == np.int64 and h.array().shape == (4, BINS) and np.array_equal(h.array(), a)
    assert (h.positions, h.units, h.saturated_units, h.pending) == (7, 3, 1, [])
    assert mod.HIST_BINS == BINS and 0 < mod.HIST_LDS_BINS < BINS
    with pytest.raises(mod.FasimError):
        mod.Hist(np.zeros((4, 100)))
    for s in ("fasim_scan_records_hist", "fasim_scan_oligos_hist", "fasim_hist_merge", "fasim_hist_free", "fasim_shuffle_query",
              "fasim_hist_threshold", "fasim_hist_tsv"):
        assert s in mod.EXPORTS and hasattr(mod.lib(), s)
