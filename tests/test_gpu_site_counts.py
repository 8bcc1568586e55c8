"""Sites per threshold on the GPU (fasim_scan_records_site_counts, fasim_scan_oligos_site_counts, k_hist_pairs): exact equality with
np.bincount over the numpy restatement of the potential (expected_potential of test_sites_cpu.py, which never calls the code under
test) and over the minima of its neighbouring positions -- slice borders, zone borders, record ends, cut / overlap pairs, record
sets, shards and their merges, values above the LDS histograms, saturation, batches, workers, the f16 switch, resident DNA,
dinucleotide controls, oligos, the CLI.  Every comparison is integer equality.  GPU only."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_sites_cpu import expected_potential, raw_runs
from test_track_cpu import same_seq
from test_gpu_track import _chromosome_like

pytestmark = pytest.mark.gpu

BINS = 16384
EXE = os.path.join(entry.PKG_DIR, "fasim")


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


def _seq(golden_dir, name):
    return synth.read_fasta(os.path.join(golden_dir, name + ".fa"))[1]


def _engine(mod, rna=None, **options):
    e = mod.Engine(0)
    for k, v in options.items():
        e.set_option(k, v)
    if rna is not None:
        e.set_query(rna)
    return e


def counts_of(P, covered=None):
    """(2, 4, 16384): the positions of a (4, n) potential of ONE record by value, and the minima of its neighbouring covered positions"""
    out = np.zeros((2, 4, BINS), dtype=np.int64)
    P = np.asarray(P, dtype=np.int64)
    cov = np.ones(P.shape[1], dtype=bool) if covered is None else covered
    both = cov[:-1] & cov[1:]
    for c in range(4):
        out[0, c] = np.bincount(P[c][cov], minlength=BINS)
        out[1, c] = np.bincount(np.minimum(P[c][:-1], P[c][1:])[both], minlength=BINS)
    return out


def _same(s, want, what=""):
    got = s.array()
    assert got.dtype == np.int64 and got.shape == (2, 4, BINS)
    if not np.array_equal(got, want):
        h, c, v = np.argwhere(got != want)[0]
        raise AssertionError((what, "pairs" if h else "positions", "class", int(c), "value", int(v), "got", int(got[h, c, v]),
                              "want", int(want[h, c, v]), "differing bins", int((got != want).sum())))


def _key(s):
    return (s.array().tolist(), s.positions, s.npairs, s.units, s.saturated_units,
            [(r, b, sd, v.tolist(), nb, link) for r, b, sd, v, nb, link in s.pending])


# ---- 1. four segments of the 30.5 kb construction x H19 ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chrom(mod, golden_dir):
    """The first 19 600 nt of the construction x H19 under rule 1, both strands (4 segments, segment 2 all N).  The restatement runs
    once per segment: P of a range is the maximum over its segments."""
    rna, dna = _seq(golden_dir, "H19"), _chromosome_like()[:19600]
    p = mod.default_params(rule=1, strand=0)
    step = p.cutLength - p.overlapLength
    nseg = mod.segment_count(len(dna), p)
    per_seg = []
    for s in range(nseg):
        P, _ = expected_potential(rna, dna, p, seg_first=s, seg_count=1)
        P.setflags(write=False)
        per_seg.append(P)

    def of_range(first, count):
        P = np.zeros((4, len(dna)), dtype=np.int64)
        cov = np.zeros(len(dna), dtype=bool)
        for s in range(first, first + count):
            P = np.maximum(P, per_seg[s])
            cov[s * step:s * step + p.cutLength] = True
        return P, cov

    P = of_range(0, nseg)[0]
    P.setflags(write=False)
    return dict(rna=rna, dna=dna, p=p, step=step, nseg=nseg, per_seg=per_seg, of_range=of_range, P=P)


def _premises(chrom):
    """The case is not vacuous; asserted on the CPU, from the restatement alone, before test_whole_record looks at the device."""
    p, step, P = chrom["p"], chrom["step"], chrom["P"]
    assert (chrom["nseg"], step, p.cutLength, len(chrom["dna"])) == (4, 4900, 5000, 19600)
    assert same_seq(chrom["dna"][2 * step:2 * step + 5000])
    sites = np.array([[len(raw_runs(P[c], v)) for v in range(0, 140)] for c in range(4)])
    total = sites.sum(axis=0)
    assert int((total[1:] > 0).sum()) >= 20
    assert (np.diff(total[1:]) > 0).any() and all((np.diff(sites[c, 1:]) > 0).any() for c in range(4))      # a site splits as v rises
    # a run that crosses a slice border of the kernel (offset 2 040 of segment 1), one that crosses the end of a head zone
    # (offset 100 of segment 1) and one that crosses the begin of a tail zone (offset 4 900 of segment 0), well above 0
    for x in (step + 2040, step + 100, step):
        assert (np.minimum(P[:, x - 1], P[:, x]) >= 30).all(), x
    # an overlap whose two segments disagree: the pairs inside a zone need the maximum of both
    assert int((chrom["per_seg"][0][:, step:step + 100] != chrom["per_seg"][1][:, step:step + 100]).sum()) > 10
    assert int(P.max()) < 512                                          # (inside the LDS histograms; case 6 leaves them)


def test_whole_record(mod, chrom):
    _premises(chrom)
    e = _engine(mod, chrom["rna"])
    res, s, ctl = e.scan_site_counts(chrom["dna"], chrom["p"])
    assert res is None and ctl == []
    want = counts_of(chrom["P"])
    _same(s, want, "whole")
    _, h, _ = e.scan_hist(chrom["dna"], chrom["p"])
    assert np.array_equal(s.array()[0], h.array())
    assert (s.positions, s.npairs, s.units, s.saturated_units, s.pending) == (19600, 19599, 12, 0, [])
    assert s.array().sum(axis=2).tolist() == [[19600] * 4, [19599] * 4]
    sites = s.sites()
    for V in (1, 20, 45, 80, int(chrom["P"].max())):
        _, st = e.scan_sites(chrom["dna"], chrom["p"], min_value=V, max_gap=0, records=False)
        rows = (st[0] if isinstance(st, (list, tuple)) else st).array()
        for c in range(4):
            assert sites[c, V] == int((rows[:, 0] == c).sum()) == len(raw_runs(chrom["P"][c], V)), (V, c)
    e.close()


# ---- 2. record lengths at every edge, for four cuts -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piece(golden_dir):
    return _seq(golden_dir, "MEG3")[400:520]


@pytest.mark.parametrize("cut,ovl", [(5000, 0), (2040, 8), (2041, 1020), (300, 150)])
def test_record_lengths_at_every_edge(mod, piece, cut, ovl):
    p = mod.default_params(rule=1, strand=0, cutLength=cut, overlapLength=ovl)
    step = cut - ovl
    lengths = sorted({n for n in (1, 2, ovl, step, step + 1, cut, cut + 1, 4950, 2 * step + 1) if n >= 1})
    big = bytearray(synth.planted_dna(sum(lengths), 31 + ovl, piece, every=150, min_len=20, max_len=60))
    dnas, at = [], 0
    for n in lengths:
        if n == 4950:
            big[at + 900:at + 1900] = b"N" * 1000                      # whole skipped segments for the short cuts
        dnas.append(bytes(big[at:at + n]))
        at += n
    wants = [counts_of(expected_potential(piece, d, p)[0]) for d in dnas]
    assert sum(int(w[1, :, 20:].sum()) for w in wants) > 50                # (neighbours that are both well above 0)
    # (the 300 / 150 cut has no segment interior at all: every pair is the host's, in any order of the batches)
    e = _engine(mod, piece, **(dict(workers=3, seg_batch=1) if cut == 300 else {}))
    _, s, _ = e.scan_site_counts(dnas, p)
    _same(s, sum(wants), "the set")                                   # pairs never span two records
    assert (s.positions, s.npairs, s.pending) == (sum(lengths), sum(lengths) - len(lengths), [])
    for n, d, w in zip(lengths, dnas, wants):
        _, s, _ = e.scan_site_counts([d], p)
        _same(s, w, f"-c {cut} -o {ovl}: record of {n} nt")
        assert (s.positions, s.npairs, s.pending) == (n, n - 1, [])
    e.close()


def test_overlap_above_half_the_cut_and_short_queries_are_refused(mod, piece):
    e = _engine(mod, piece)
    dna = synth.random_dna(1000, 5)
    bad = mod.default_params(rule=1, strand=0, cutLength=301, overlapLength=151)
    with pytest.raises(mod.FasimError) as ei:
        e.scan_site_counts(dna, bad)
    assert ei.value.code == mod.E_UNSUPPORTED
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_site_counts([b"GGAGGAGGGAAGGAGGGAGG"], dna, bad)
    assert ei.value.code == mod.E_UNSUPPORTED
    p = mod.default_params(rule=1, strand=0)
    refusal = None
    try:
        e.scan_hist(dna, p, rnas=[piece[:112]])
    except mod.FasimError as x:
        refusal = x.code
    assert refusal is not None
    with pytest.raises(mod.FasimError) as ei:
        e.scan_site_counts(dna, p, rnas=[piece[:112]])                 # the lncRNA call takes 113 nt or more, as scan_hist()
    assert ei.value.code == refusal
    with pytest.raises(mod.FasimError):
        e.scan_site_counts(dna, p, shuffle="tri")
    e.set_query(piece)
    _, s, _ = e.scan_site_counts(dna, p)                              # the engine is usable afterwards
    e.close()
    _same(s, counts_of(expected_potential(piece, dna, p)[0]), "after the refusals")


# ---- 3. record sets -------------------------------------------------------------------------------------------------------------------
def test_record_sets(mod, chrom):
    dna, p = chrom["dna"], chrom["p"]
    recs = [dna[:5100], dna[4000:9000], dna[14700:17000]]
    e = _engine(mod, chrom["rna"])
    _, whole, _ = e.scan_site_counts(recs, p)
    alone = [e.scan_site_counts([r], p)[1] for r in recs]
    e.close()
    assert np.array_equal(whole.array(), sum(a.array() for a in alone))
    assert (whole.positions, whole.npairs, whole.pending) == (sum(map(len, recs)), sum(map(len, recs)) - 3, [])
    _same(alone[0], counts_of(expected_potential(chrom["rna"], recs[0], p)[0]), "record 0")


# ---- 4. shards ------------------------------------------------------------------------------------------------------------------------
def test_shards_and_their_merges(mod, chrom):
    e = _engine(mod, chrom["rna"])
    nseg, step = chrom["nseg"], chrom["step"]
    _, whole, _ = e.scan_site_counts(chrom["dna"], chrom["p"])
    shard = {}

    def get(first, count):
        if (first, count) not in shard:
            _, s, _ = e.scan_site_counts(chrom["dna"], chrom["p"], seg_first=first, seg_count=count)
            P, cov = chrom["of_range"](first, count)
            _same(s, counts_of(P, cov), f"shard {first}+{count}")
            assert s.positions == int(cov.sum()) and s.npairs == s.positions - 1
            want_edges = ([(0, first - 1, 1)] if first > 0 else []) + ([(0, first + count - 1, 0)] if first + count < nseg else [])
            assert [(r, b, sd) for r, b, sd, _, _, _ in s.pending] == want_edges       # a lone shard has pending edges
            for r, b, sd, v, nb, link in s.pending:
                a = (b + 1) * step
                assert np.array_equal(v, P[:, a:a + 100]) and link == 1 and nb == P[:, a - 1 if sd == 0 else a + 100].tolist()
            shard[(first, count)] = s
        return shard[(first, count)]

    for k in range(1, nseg):                                          # (k = 2 and k = 3 cut beside the all-N segment)
        a, b = get(0, k), get(k, nseg - k)
        assert _key(mod.merge_site_counts([a, b])) == _key(whole) == _key(mod.merge_site_counts([b, a])), k
    for i, j in ((1, 2), (1, 3), (2, 3)):
        parts = [get(0, i), get(i, j - i), get(j, nseg - j)]
        for perm in itertools.permutations(range(3)):
            x, y, z = (parts[t] for t in perm)
            assert _key(mod.merge_site_counts([x, y, z])) == _key(whole), (i, j, perm)
            assert _key(mod.merge_site_counts([mod.merge_site_counts([x, y]), z])) == _key(whole), (i, j, perm)
    e.close()


# ---- 5. invariance --------------------------------------------------------------------------------------------------------------------
def test_batches_workers_f16_resident_and_records(mod, chrom, golden_dir):
    want = counts_of(chrom["P"])
    for options in (dict(workers=1, dp_f16=0), dict(workers=3, seg_batch=1, dp_f16=1), dict(seg_batch=2)):
        e = _engine(mod, chrom["rna"], **options)
        _, s, _ = e.scan_site_counts(chrom["dna"], chrom["p"])
        _same(s, want, str(options))
        assert (s.positions, s.units, s.pending) == (19600, 12, [])
        e.close()
    e = _engine(mod, chrom["rna"], seg_batch=3)
    e.load_dna(chrom["dna"])
    _, s, _ = e.scan_site_counts(None, chrom["p"])
    _same(s, want, "resident")
    res, s, _ = e.scan_site_counts(chrom["dna"], chrom["p"], records=True)
    _same(s, want, "with stage 3")
    assert len(res) == 1
    # (H19 leaves no triplex on this record under rule 1; MEG3 on the whole construction does, as in test_gpu_hist.py)
    e.set_query(_seq(golden_dir, "MEG3"))
    dna = _chromosome_like()
    plain = e.scan_records([dna], chrom["p"])
    _, alone, _ = e.scan_site_counts(dna, chrom["p"])
    res, s, _ = e.scan_site_counts(dna, chrom["p"], records=True)
    assert _key(s) == _key(alone)
    x, y = res[0], plain[0]
    assert y.count > 0 and (x.count, x.recs, x.pool) == (y.count, y.recs, y.pool)
    e.close()


# ---- 6. values above the LDS histograms, saturation ----------------------------------------------------------------------------------------
def test_values_above_the_lds_histograms(mod, golden_dir):
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    dna = synth.planted_dna(5000, 41, rna, min_len=1300, max_len=1300, mut_pct=0, indel_pct=0)
    P, _ = expected_potential(rna, dna, p)
    want = counts_of(P)
    assert int(P.max()) >= 1024 and int(want[1, :, 1024:].sum()) > 0 and int(want[1, :, mod.HIST_PAIR_LDS_BINS:1024].sum()) > 0
    e = _engine(mod, rna)
    _, s, _ = e.scan_site_counts(dna, p)
    e.close()
    _same(s, want, "planted copy")
    assert (s.positions, s.npairs, s.units, s.saturated_units) == (5000, 4999, 2 * 48, 0)


def test_saturated_units(mod, golden_dir):
    """Against the unchanged scan_track(bin = 1), as test_gpu_hist.py: a perfect copy of 3 400 nt of MALAT1 saturates the potential."""
    p = mod.default_params()
    rna = _seq(golden_dir, "MALAT1")
    dna = synth.planted_dna(5000, 65, rna, min_len=3400, max_len=3400, mut_pct=0, indel_pct=0)
    e = _engine(mod, rna)
    _, t = e.scan_track(dna, p, bin=1, records=False)
    _, s, _ = e.scan_site_counts(dna, p)
    e.close()
    track = t.array().astype(np.int64)
    assert int(track.max()) == 16383 and t.saturated_units >= 1
    want = counts_of(track)
    assert int(want[1, :, 16383].sum()) > 0
    _same(s, want, "planted 3 400 nt of MALAT1")
    assert (s.saturated_units, s.units, s.positions) == (t.saturated_units, t.units, len(dna))


# ---- 7. controls ----------------------------------------------------------------------------------------------------------------------
def test_dinucleotide_controls_are_plain_queries(mod, chrom):
    rna = chrom["rna"]
    dna, p = chrom["dna"][:9000], chrom["p"]
    e = _engine(mod, rna)
    _, s, ctl = e.scan_site_counts(dna, p, controls=2, seed=7, shuffle="di")
    assert len(ctl) == 2 and e.m == len(rna)
    _, alone, none = e.scan_site_counts(dna, p)
    assert _key(s) == _key(alone) and none == []
    shuffled = [mod.shuffle_query_dinuc(rna, 7, k) for k in (1, 2)]
    assert len(set(shuffled + [rna])) == 3
    for k, q in enumerate(shuffled):
        e.set_query(q)
        assert _key(ctl[k]) == _key(e.scan_site_counts(dna, p)[1]), k
    _same(ctl[0], counts_of(expected_potential(shuffled[0], dna, p)[0]), "control 1 against the restatement")
    e.set_query(rna)
    _, _, mono = e.scan_site_counts(dna, p, controls=1, seed=7)
    e.set_query(mod.shuffle_query(rna, 7, 1))
    assert _key(mono[0]) == _key(e.scan_site_counts(dna, p)[1])
    e.close()
    v = mod.site_counts_threshold(s, ctl, 0.05)
    assert v >= 0
    head = mod.site_counts_tsv(s, "H19", ctl, seed=7, shuffle="di").split(b"\n")[0].decode()
    assert head == f"# fasim site counts lncRNA=H19 positions=9000 controls=2 seed=7 shuffle=di fdr=0.05 min_value={v if v else 'NA'}"


# ---- 8. oligos ------------------------------------------------------------------------------------------------------------------------
def test_oligo_panels(mod, golden_dir):
    meg3 = _seq(golden_dir, "MEG3")
    oligos = [meg3[700:720], meg3[700:812]]
    assert [len(o) for o in oligos] == [20, 112]
    p = mod.default_params(rule=1, strand=0)
    dnas = [synth.planted_dna(9950, 51, meg3[690:830], every=250, min_len=18, max_len=110), synth.random_dna(4950, 52)]
    e = _engine(mod)
    cs = e.scan_oligos_site_counts(oligos, dnas, p)
    _, tracks = e.scan_oligos(oligos, dnas, p, min_value=1, track_bin=1)
    for q, o in enumerate(oligos):
        want = sum(counts_of(t.array()) for t in tracks[q])
        _same(cs[q], want, f"{len(o)}-nt oligo against its tracks")
        assert (cs[q].positions, cs[q].npairs, cs[q].pending) == (9950 + 4950, 9950 + 4950 - 2, [])
    _same(cs[0], sum(counts_of(expected_potential(oligos[0], d, p)[0]) for d in dnas), "20-nt oligo against the restatement")
    parts = [e.scan_oligos_site_counts(oligos, dnas, p, seg_first=a, seg_count=n) for a, n in ((0, 2), (2, 1), (3, 2))]
    for q in range(2):
        assert _key(mod.merge_site_counts([x[q] for x in parts])) == _key(cs[q]), q
    with pytest.raises(mod.FasimError) as ei:
        e.scan_oligos_site_counts([meg3[:113]], dnas, p)
    assert ei.value.code == mod.E_ARG
    e.close()


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------------
def _run(wd, *args, status=0):
    r = subprocess.run([EXE, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    assert r.returncode == status, r.stderr
    return r


def _files(d):
    return {n: (d / n).read_bytes() for n in sorted(os.listdir(d))}


def _min_value(table):
    v = table.splitlines()[0].decode().rsplit("min_value=", 1)[1]
    return 0 if v == "NA" else int(v)


def test_cli_plain_run_and_refusals(mod, golden_dir, tmp_path):
    for f in ("H19.fa", "testDNA.fa"):
        (tmp_path / f).write_bytes(open(os.path.join(golden_dir, f), "rb").read())
    rna, dna = _seq(golden_dir, "H19"), _seq(golden_dir, "testDNA")
    p = mod.default_params(cLength=40)
    e = _engine(mod, rna)
    _, s, ctl = e.scan_site_counts(dna, p, controls=2, seed=5)
    _, sd, ctld = e.scan_site_counts(dna, p, controls=2, seed=5, shuffle="di")
    e.close()
    name, hname = "hg19-H19-testDNA-TFOsitecounts", "hg19-H19-testDNA-TFOhist"

    def run(out, *extra, status=0):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", "testDNA.fa", "-f2", "H19.fa", "-O", out + "/", "-lg", "40", *extra, status=status)
        return _files(tmp_path / out)

    ctl_args = ("--hist-controls", "2", "--hist-seed", "5", "--hist-fdr", "0.2")
    # the reference's three files and the hist table are what they are without --hist-sites
    base = run("base", "--potential-hist", *ctl_args)
    assert len(base) == 4 and hname in base
    want = mod.site_counts_tsv(s, "H19", ctl, seed=5, fdr=0.2)
    assert want.startswith(b"# fasim site counts lncRNA=H19 positions=%d controls=2 seed=5 shuffle=mono fdr=0.2 min_value=" % len(dna))
    got = run("sites", "--potential-hist", "--hist-sites", *ctl_args)
    assert got == dict(base, **{name: want})
    assert _min_value(got[name]) == mod.site_counts_threshold(s, ctl, 0.2)
    assert run("mono", "--potential-hist", "--hist-sites", "--hist-shuffle", "mono", *ctl_args) == got
    assert run("two", "--potential-hist", "--hist-sites", *ctl_args, "--devices", "0,0") == got
    assert run("none", "--potential-hist", "--hist-sites") == dict(run("none0", "--potential-hist"), **{name: mod.site_counts_tsv(s, "H19")})
    # --hist-shuffle di reaches both tables
    wantd = mod.site_counts_tsv(sd, "H19", ctld, seed=5, fdr=0.2, shuffle="di")
    gotd = run("di", "--potential-hist", "--hist-sites", "--hist-shuffle", "di", "--potential-hist-only", *ctl_args)
    hd = mod.hist_tsv(mod.Hist(sd.array()[0]), "H19", [mod.Hist(c.array()[0]) for c in ctld], seed=5, fdr=0.2)
    assert gotd == {hname: hd, name: wantd} and b" shuffle=di " in wantd.splitlines()[0]
    assert _min_value(gotd[name]) == mod.site_counts_threshold(sd, ctld, 0.2)
    assert run("di0", "--potential-hist", "--hist-shuffle", "di", "--potential-hist-only", *ctl_args) == {hname: hd}
    for k, extra in enumerate((["--hist-sites"], ["--hist-shuffle", "di"], ["--potential-hist", "--hist-shuffle", "tri"],
                               ["--potential-hist", "--hist-sites", "--hist-shuffle", "Di"])):
        assert run(f"refused{k}", *extra, status=2) == {}, extra


def test_cli_record_sets_and_oligos(mod, golden_dir, tmp_path):
    import helpers
    peaks = helpers.read_peaks(os.path.join(golden_dir, "meg3_peaks.fa.gz"))[:6]
    (tmp_path / "MEG3.fa").write_bytes(open(os.path.join(golden_dir, "MEG3.fa"), "rb").read())
    lnc = synth.read_fasta(str(tmp_path / "MEG3.fa"))[0]
    rna = _seq(golden_dir, "MEG3")
    p = mod.default_params()
    recs = [x for _, x in peaks]
    (tmp_path / "recs.fa").write_bytes(b"".join(f">{h}\n".encode() + x + b"\n" for h, x in peaks))
    e = _engine(mod, rna)
    _, s, ctl = e.scan_site_counts(recs, p, controls=2, seed=3, shuffle="di")
    e.close()
    want = mod.site_counts_tsv(s, lnc, ctl, seed=3, shuffle="di")

    def run(out, f1, f2, *extra):
        (tmp_path / out).mkdir()
        _run(tmp_path, "-f1", f1, "-f2", f2, "-O", out + "/", *extra)
        return _files(tmp_path / out)

    args = ("--all-records", "--potential-hist", "--hist-controls", "2", "--hist-seed", "3", "--hist-shuffle", "di")
    fname = f"{lnc}-recs.sitecounts.tsv"
    base = run("base", "recs.fa", "MEG3.fa", *args)
    assert len(base) == 3 * len(peaks) + 1 and f"{lnc}-recs.hist.tsv" in base
    got = run("all", "recs.fa", "MEG3.fa", *args, "--hist-sites")
    assert got == dict(base, **{fname: want})
    assert _min_value(got[fname]) == mod.site_counts_threshold(s, ctl, 0.05)
    assert run("all2", "recs.fa", "MEG3.fa", *args, "--hist-sites", "--devices", "0,0") == got
    # --oligos: one table per oligo beside its hist table
    oligos, names = [rna[700:720], rna[700:812]], ["tfo20", "tfo112"]
    (tmp_path / "panel.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), o) for n, o in zip(names, oligos)))
    e = _engine(mod)
    cs = e.scan_oligos_site_counts(oligos, recs, p)
    cc = [e.scan_oligos_site_counts([mod.shuffle_query_dinuc(o, 3, k) for k in (1, 2)], recs, p) for o in oligos]
    e.close()
    obase = run("obase", "recs.fa", "panel.fa", "--oligos", *args)
    assert sorted(obase) == sorted(f"{n}-recs.hist.tsv" for n in names)
    wanto = {f"{n}-recs.sitecounts.tsv": mod.site_counts_tsv(cs[q], n, cc[q], seed=3, shuffle="di") for q, n in enumerate(names)}
    assert run("oligos", "recs.fa", "panel.fa", "--oligos", *args, "--hist-sites") == dict(obase, **wanto)
    for q, n in enumerate(names):
        assert _min_value(wanto[f"{n}-recs.sitecounts.tsv"]) == mod.site_counts_threshold(cs[q], cc[q], 0.05)
