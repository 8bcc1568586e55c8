"""Sites per threshold with dinucleotide controls, the part that needs no GPU: the pure host functions of the
C-ABI -- fasim_shuffle_query_dinuc, fasim_site_counts_merge, fasim_site_counts_threshold, fasim_site_counts_tsv -- and the identity
behind SiteCounts.sites(), against restatements of their definitions written here, which never call the code under test."""
import itertools
import os
from collections import Counter

import numpy as np
import pytest

import __graft_entry__ as entry
import synth
from test_sites_cpu import raw_runs

BINS = 16384
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


# ---- the dinucleotide shuffle --------------------------------------------------------------------------------------------------------
def dinuc_restated(rna: bytes, seed: int, k: int) -> bytes:
    m = len(rna)
    if m < 3:
        return bytes(rna)
    state = [(seed ^ (k * 0xD1B54A32D192ED03)) & MASK]

    def nxt():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & MASK
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    z = rna[-1]
    succ = {}
    for x, y in zip(rna, rna[1:]):
        succ.setdefault(x, []).append(y)
    order = sorted(succ)
    while True:
        last = {a: nxt() % len(succ[a]) for a in order if a != z}
        ok = True
        for a in last:
            w, steps = a, 0
            while w != z and steps <= 256:
                w = succ[w][last[w]]
                steps += 1
            ok = ok and w == z
        if ok:
            break
    for a in order:
        lst = succ[a]
        free = len(lst)
        if a != z:
            lst.append(lst.pop(last[a]))
            free -= 1
        for i in range(free - 1, 0, -1):
            j = nxt() % (i + 1)
            lst[i], lst[j] = lst[j], lst[i]
    out, w, used = bytearray([rna[0]]), rna[0], Counter()
    for _ in range(m - 1):
        nw = succ[w][used[w]]
        used[w] += 1
        w = nw
        out.append(w)
    return bytes(out)


def _h19(golden_dir):
    return synth.read_fasta(os.path.join(golden_dir, "H19.fa"))[1]


def test_dinuc_shuffle_equals_the_restatement(mod, golden_dir):
    h19 = _h19(golden_dir)
    rng = np.random.default_rng(5)
    cases = [bytes(rng.choice(np.frombuffer(b"ACGUTacgunN", dtype=np.uint8), size=m).tobytes()) for m in (1, 2, 3, 17)]
    cases += [h19, h19.replace(b"T", b"U").lower()[:900] + b"NNnACGU", b"AAAAAAA", b"ACACACAG"]
    assert len(h19) > 2000
    for rna in cases:
        for seed, k in ((0, 1), (0, 2), (7, 1), (7, 3), (2 ** 64 - 1, 1), (0x123456789ABCDEF0, 40000)):
            got = mod.shuffle_query_dinuc(rna, seed, k)
            assert got == dinuc_restated(rna, seed, k), (len(rna), seed, k)
            assert Counter(zip(got, got[1:])) == Counter(zip(rna, rna[1:])) and Counter(got) == Counter(rna)
            assert got[:1] == rna[:1] and got[-1:] == rna[-1:]
    # a single Euler path: the repeat that a mononucleotide shuffle destroys comes back as it is
    ga = b"GA" * 40
    assert mod.shuffle_query_dinuc(ga, 3, 1) == ga and mod.shuffle_query(ga, 3, 1) != ga
    r200 = synth.random_dna(200, 9)
    assert mod.shuffle_query_dinuc(r200, 7, 1) != r200 and mod.shuffle_query_dinuc(r200, 7, 1) != mod.shuffle_query_dinuc(r200, 7, 2)
    assert mod.shuffle_query_dinuc(h19, 7, 1) != h19
    for bad in ((b"", 0, 1), (b"ACGT", 0, 0)):
        with pytest.raises(mod.FasimError) as ei:
            mod.shuffle_query_dinuc(*bad)
        assert ei.value.code == mod.E_ARG


# ---- the identity --------------------------------------------------------------------------------------------------------------------
def counts_of(P, covered=None):
    """(2, 4, 16384): bincount of a (4, n) potential of ONE record over its covered positions, and of the minima of its neighbouring
    covered positions."""
    out = np.zeros((2, 4, BINS), dtype=np.int64)
    cov = np.ones(P.shape[1], dtype=bool) if covered is None else covered
    both = cov[:-1] & cov[1:]
    for c in range(4):
        out[0, c] = np.bincount(P[c][cov], minlength=BINS)
        out[1, c] = np.bincount(np.minimum(P[c][:-1], P[c][1:])[both], minlength=BINS)
    return out


def test_sites_are_positions_minus_pairs(mod):
    rng = np.random.default_rng(11)
    rising = 0
    for n, top in ((1, 5), (2, 5), (50, 3), (400, 12), (3000, 40), (3000, 2)):
        P = rng.integers(0, top + 1, size=(4, n)).astype(np.int64)
        P[:, rng.random(n) < 0.5] = 0
        if n == 400:
            P[0, :12] = [0, 5, 5, 9, 2, 9, 5, 0, 0, 3, 3, 0]          # one site at 2, two at 3 .. 5 and two at 6 .. 9
            P[1, 100] = 16383
        sc = mod.SiteCounts(counts_of(P))
        sites = sc.sites()
        assert sites.shape == (4, BINS) and sites.dtype == np.int64 and (sc.positions, sc.npairs) == (n, n - 1)
        for c in range(4):
            for v in list(range(1, top + 2)) + [16383]:
                assert sites[c, v] == len(raw_runs(P[c], v)), (n, c, v)
            rising += int((np.diff(sites[c, 1:top + 2]) > 0).sum())
    assert rising > 0                                                  # sites is not monotone: a site splits as the threshold rises


# ---- the merge -----------------------------------------------------------------------------------------------------------------------
def _toy_records(cut, ovl, lens, seed=17):
    """Records of the given lengths, per segment a (4, len) array of its own values; segment 2 of record 0 is 'skipped' (zeros)."""
    rng = np.random.default_rng(seed)
    step = cut - ovl
    recs = []
    for n in lens:
        segs = [rng.integers(0, 6, size=(4, min(cut, n - a))).astype(np.uint16) for a in range(0, n, step)]
        recs.append((n, segs))
    if len(recs[0][1]) > 2:
        recs[0][1][2][:] = 0
    return recs


def _toy_counts(mod, recs, cut, ovl, first, count):
    """The site counts of global segments [first, first + count) by the definition, and a pending edge for every boundary with
    exactly one side selected: its own zone values, and the range's value at the position next to the zone."""
    step = cut - ovl
    counts = np.zeros((2, 4, BINS), dtype=np.int64)
    pending, g, units = [], 0, 0
    for r, (n, segs) in enumerate(recs):
        P = np.zeros((4, n), dtype=np.int64)
        cov = np.zeros(n, dtype=bool)
        sel = [first <= g + i < first + count for i in range(len(segs))]
        for i, v in enumerate(segs):
            if sel[i]:
                a = i * step
                P[:, a:a + v.shape[1]] = np.maximum(P[:, a:a + v.shape[1]], v)
                cov[a:a + v.shape[1]] = True
                units += 1
        for b in range(len(segs) - 1):
            if sel[b] == sel[b + 1]:
                continue
            ln = min(ovl, segs[b + 1].shape[1])
            a = (b + 1) * step                                          # the zone is [a, a + ln)
            if sel[b]:
                head = ovl if b > 0 else 0                              # (segment b has a successor: its tail zone starts at `step`)
                link = 1 if step - 1 >= head else 2
                pending.append((r, b, 0, segs[b][:, step:step + ln], P[:, a - 1].tolist(), link))
            else:
                L = segs[b + 1].shape[1]
                tail = step if b + 2 < len(segs) else L
                link = 0 if ln >= L else 1 if ln < tail else 2
                pending.append((r, b, 1, segs[b + 1][:, :ln], P[:, a + ln].tolist() if link else [0] * 4, link))
        counts += counts_of(P, cov)
        g += len(segs)
    return mod.SiteCounts(counts, units=units, saturated_units=count, pending=pending)


def _key(s):
    return (s.array().tolist(), s.positions, s.npairs, s.units, s.saturated_units,
            [(r, b, sd, v.tolist(), nb, link) for r, b, sd, v, nb, link in s.pending])


# cut, overlap, record lengths: 4 segments + 2; the last segment of record 0 inside its head zone; no interior at all (2 ovl == cut)
TOYS = [(10, 0, (37, 12)), (10, 1, (30, 12)), (20, 8, (45, 30)), (20, 8, (41, 30)), (20, 8, (44, 12)), (16, 8, (32, 20)), (16, 8, (30, 17))]


@pytest.mark.parametrize("cut,ovl,lens", TOYS)
def test_merge_pairs_the_pending_edges(mod, cut, ovl, lens):
    recs = _toy_records(cut, ovl, lens)
    step = cut - ovl
    nseg0, nseg = len(recs[0][1]), sum(len(s) for _, s in recs)
    assert nseg0 == 4
    if (cut, ovl, lens[0]) in ((20, 8, 41), (20, 8, 44), (16, 8, 32)):
        assert recs[0][1][3].shape[1] <= ovl                            # the last segment lies wholly inside its head zone
    whole = _toy_counts(mod, recs, cut, ovl, 0, nseg)
    assert (whole.positions, whole.npairs, whole.pending) == (sum(lens), sum(lens) - len(lens), [])
    full = np.zeros((2, 4, BINS), dtype=np.int64)
    for n, segs in recs:
        P = np.zeros((4, n), dtype=np.int64)
        for i, v in enumerate(segs):
            P[:, i * step:i * step + v.shape[1]] = np.maximum(P[:, i * step:i * step + v.shape[1]], v)
        full += counts_of(P)
    assert np.array_equal(whole.array(), full)
    one = [_toy_counts(mod, recs, cut, ovl, s, 1) for s in range(nseg)]
    assert sum(h.array() for h in one).tolist() != whole.array().tolist()
    # two parts, cut at every boundary, both orders
    for k in range(1, nseg):
        a, b = _toy_counts(mod, recs, cut, ovl, 0, k), _toy_counts(mod, recs, cut, ovl, k, nseg - k)
        assert len(a.pending) == len(b.pending) == (0 if k == nseg0 else 1)
        for parts in ((a, b), (b, a)):
            assert _key(mod.merge_site_counts(parts)) == _key(whole), k
    # three parts, every order and nesting; partial merges are the counts of the union, pending edges included
    for i, j in itertools.combinations(range(1, nseg), 2):
        parts = [_toy_counts(mod, recs, cut, ovl, 0, i), _toy_counts(mod, recs, cut, ovl, i, j - i), _toy_counts(mod, recs, cut, ovl, j, nseg - j)]
        for perm in itertools.permutations(range(3)):
            x, y, z = (parts[t] for t in perm)
            assert _key(mod.merge_site_counts([x, y, z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_site_counts([mod.merge_site_counts([x, y]), z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_site_counts([x, mod.merge_site_counts([y, z])])) == _key(whole), (i, j, perm)
        assert _key(mod.merge_site_counts(parts[:2])) == _key(_toy_counts(mod, recs, cut, ovl, 0, j)), (i, j)
        assert _key(mod.merge_site_counts(parts[1:])) == _key(_toy_counts(mod, recs, cut, ovl, i, nseg - i)), (i, j)
        outer = mod.merge_site_counts([parts[0], parts[2]])            # not neighbours: nothing pairs
        assert outer.positions == parts[0].positions + parts[2].positions and outer.npairs == parts[0].npairs + parts[2].npairs
        assert len(outer.pending) == len(parts[0].pending) + len(parts[2].pending)
    # all single segments, in several orders
    for order in (one, one[::-1], one[1::2] + one[::2], [one[2], one[0], one[3], one[1]] + one[4:]):
        assert _key(mod.merge_site_counts(order)) == _key(whole)
    assert _key(mod.merge_site_counts([whole])) == _key(whole)


def test_merge_refusals(mod):
    recs = _toy_records(20, 8, (45, 30))
    a = _toy_counts(mod, recs, 20, 8, 0, 2)
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_counts([a, a])                                  # the same edge pending twice: the parts overlap
    assert ei.value.code == mod.E_ARG
    z = np.zeros((2, 4, BINS), dtype=np.int64)
    x = mod.SiteCounts(z, pending=[(0, 1, 0, np.zeros((4, 3)), [0] * 4, 1)])
    y = mod.SiteCounts(z, pending=[(0, 1, 1, np.zeros((4, 2)), [0] * 4, 1)])
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_counts([x, y])
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_counts([mod.SiteCounts(z, pending=[(0, 1, 0, np.zeros((4, 3)), [0] * 4, 3)])])      # no such link
    assert ei.value.code == mod.E_ARG
    with pytest.raises(mod.FasimError) as ei:
        mod.merge_site_counts([])
    assert ei.value.code == mod.E_ARG


# ---- the threshold -------------------------------------------------------------------------------------------------------------------
def _counts_of_rows(mod, rows):
    """rows: {class: [potential per position]} of one record of equal length per class"""
    n = max(len(v) for v in rows.values())
    P = np.zeros((4, n), dtype=np.int64)
    for c, v in rows.items():
        P[c, :len(v)] = v
    return mod.SiteCounts(counts_of(P))


def site_threshold_restated(real, controls, Q):
    K = len(controls)
    s = real.sites().sum(axis=0)
    cs = sum((c.sites().sum(axis=0) for c in controls), np.zeros(BINS, dtype=np.int64))
    for v in range(1, BINS):
        if s[v] > 0 and all(float(cs[w]) <= Q * K * float(s[w]) for w in range(v, BINS) if s[w] > 0):
            return v
    return 0


def test_threshold_on_hand_made_curves(mod):
    # 1 site at 1 .. 2, 20 sites at 3 .. 5 (one long site splits), 3 at 6 .. 9; positions would say otherwise
    real = _counts_of_rows(mod, {0: [2] + [5, 2] * 17 + [0, 9, 0, 9, 0], 2: [0] * 10 + [9] * 30})
    assert real.sites().sum(axis=0)[[1, 2, 3, 5, 6, 9, 10]].tolist() == [4, 4, 20, 20, 3, 3, 0]
    ctl = [_counts_of_rows(mod, {1: [0, 7, 0, 4, 0] + [0] * 40}), _counts_of_rows(mod, {3: [0, 3, 3, 3, 0, 1] + [0] * 39})]
    for q in (0.001, 0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 1.0):
        assert mod.site_counts_threshold(real, ctl, q) == site_threshold_restated(real, ctl, q), q
    # at 6 .. 7 one control site against 3: 1 > 0.1 * 2 * 3 fails, so the answer lies above; at 3: 3 <= 0.1 * 2 * 20
    assert mod.site_counts_threshold(real, ctl, 0.1) == 8 and mod.site_counts_threshold(real, ctl, 0.2) == 3
    assert mod.site_counts_threshold(real, ctl, 1.0) == 1 and mod.site_counts_threshold(real, [], 0.05) == 1
    assert mod.site_counts_threshold(real, [real], 0.05) == site_threshold_restated(real, [real], 0.05) == 0
    flat = _counts_of_rows(mod, {0: [0] * 10})
    assert mod.site_counts_threshold(flat, [], 0.05) == 0 and mod.site_counts_threshold(flat, [flat], 0.05) == 0
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(mod.FasimError) as ei:
            mod.site_counts_threshold(real, ctl, bad)
        assert ei.value.code == mod.E_ARG


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_tsv_bytes(mod):
    real = _counts_of_rows(mod, {0: [0, 2, 4, 2, 0, 2, 0, 0], 2: [1, 0, 0, 0, 0, 0, 0, 1], 3: [4, 4, 0, 4, 0, 0, 0, 0]})
    head = "value\tParaPlus_sites\tParaMinus_sites\tAntiMinus_sites\tAntiPlus_sites\tall_sites\n"
    want = "# fasim site counts lncRNA=MEG3 positions=8\n" + head + "1\t2\t0\t2\t2\t6\n2\t2\t0\t0\t2\t4\n3\t1\t0\t0\t2\t3\n4\t1\t0\t0\t2\t3\n"
    assert mod.site_counts_tsv(real, "MEG3") == want.encode()
    ctl = [_counts_of_rows(mod, {0: [1, 0, 0, 0, 0, 0, 0, 0]}), _counts_of_rows(mod, {1: [0, 6, 0, 0, 0, 0, 0, 0]})]
    headc = ("value\tParaPlus_sites\tParaPlus_ctl_sites\tParaMinus_sites\tParaMinus_ctl_sites\tAntiMinus_sites\tAntiMinus_ctl_sites\t"
             "AntiPlus_sites\tAntiPlus_ctl_sites\tall_sites\tall_ctl_sites\tfdr\n")
    wantc = ("# fasim site counts lncRNA=MEG3 positions=8 controls=2 seed=7 shuffle=di fdr=0.1 min_value=NA\n" + headc +
             "1\t2\t1\t0\t1\t2\t0\t2\t0\t6\t2\t0.166667\n"
             "2\t2\t0\t0\t1\t0\t0\t2\t0\t4\t1\t0.125\n"
             "3\t1\t0\t0\t1\t0\t0\t2\t0\t3\t1\t0.166667\n"
             "4\t1\t0\t0\t1\t0\t0\t2\t0\t3\t1\t0.166667\n"
             "5\t0\t0\t0\t1\t0\t0\t0\t0\t0\t1\tNA\n"
             "6\t0\t0\t0\t1\t0\t0\t0\t0\t0\t1\tNA\n")
    assert mod.site_counts_tsv(real, "MEG3", ctl, seed=7, fdr=0.1, shuffle="di") == wantc.encode()
    assert mod.site_counts_tsv(real, "MEG3", ctl, seed=7, fdr=0.25, shuffle="mono") == \
        wantc.replace("shuffle=di fdr=0.1 min_value=NA", "shuffle=mono fdr=0.25 min_value=1").encode()
    empty = _counts_of_rows(mod, {0: [0] * 5})
    assert mod.site_counts_tsv(empty, "q") == ("# fasim site counts lncRNA=q positions=5\n" + head).encode()
    with pytest.raises(mod.FasimError):
        mod.site_counts_tsv(real, "q", shuffle="tri")


def test_site_counts_object_and_symbols(mod):
    a = np.zeros((2, 4, BINS), dtype=np.int64)
    a[0, :, 0] = 7
    a[1, :, 0] = 6
    a[0, 2, 16383], a[0, 2, 0] = 2, 5
    s = mod.SiteCounts(a, units=3, saturated_units=1)
    assert s.array().dtype == np.int64 and s.array().shape == (2, 4, BINS) and np.array_equal(s.array(), a)
    assert (s.positions, s.npairs, s.units, s.saturated_units, s.pending) == (7, 6, 3, 1, [])
    assert s.sites()[2, 16383] == 2 and s.sites()[:, 0].tolist() == [1, 1, 1, 1]
    assert 0 < mod.HIST_PAIR_LDS_BINS <= mod.HIST_LDS_BINS
    with pytest.raises(mod.FasimError):
        mod.SiteCounts(np.zeros((4, BINS)))
    for name in ("fasim_scan_records_site_counts", "fasim_scan_oligos_site_counts", "fasim_site_counts_merge", "fasim_site_counts_free",
                 "fasim_shuffle_query_dinuc", "fasim_site_counts_threshold", "fasim_site_counts_tsv"):
        assert name in mod.EXPORTS and hasattr(mod.lib(), name)
    for name in ("SiteCounts", "merge_site_counts", "site_counts_threshold", "site_counts_tsv", "shuffle_query_dinuc"):
        assert hasattr(mod, name)
    for name in ("scan_site_counts", "scan_oligos_site_counts"):
        assert hasattr(mod.Engine, name)
