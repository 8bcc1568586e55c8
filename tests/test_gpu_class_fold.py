"""The front half that k_track, k_sites and k_hist share (class_fold.h), through every consumer on the same inputs: record lengths
that put the segment end -- and with it the mirror's first column, its last column and its first aligned group of 8 -- on every
side of a lane's group of 8 and of a slice of 2 040 positions, under three class tables.  Tracks, peaks, sites and histogram equal
the numpy restatement (test_track_cpu.py / test_sites_cpu.py, which never call the code under test) and agree with one another.
Every comparison is integer equality.  GPU only.

The class tables: an even encoding is read forward and an odd one reversed, and the class of an encoding follows its parity too
(enc_class), so under EVERY -r / -t setting ParaPlus and AntiMinus hold forward rows only and ParaMinus and AntiPlus reversed
rows only: groups (ParaPlus, reversed), (ParaMinus, forward), (AntiMinus, reversed) and (AntiPlus, forward) are always empty.  The
three settings differ in the other four: one row each; six rows in the two Para groups and none in the Anti groups; one row in
the two Anti groups and none in the Para groups."""
import os

import numpy as np
import pytest

import synth
import __graft_entry__ as entry
from test_gpu_hist import bincount4
from test_gpu_sites import _same
from test_sites_cpu import expected_potential, sites_from
from test_track_cpu import bin_reduce, enabled_encodings, enc_class

pytestmark = pytest.mark.gpu

# one segment each (the default cut is 5 000) ... and one record of three segments (step 4 900, overlaps of 100)
LENGTHS = (1, 7, 8, 9, 2039, 2040, 2041, 2047, 2048, 4079, 4080, 4081, 5000) + (9900,)
SEED = 31
# (rule, strand) -> rows per group g = class + 4 * reversed
SETTINGS = {(1, 0): [1, 0, 1, 0, 0, 1, 0, 1], (0, 1): [6, 0, 0, 0, 0, 6, 0, 0], (2, -1): [0, 0, 1, 0, 0, 0, 0, 1]}


@pytest.fixture(scope="module")
def mod():
    if not os.path.exists(os.path.join(entry.PKG_DIR, "libfasim_hip.so")):
        entry.build()
    return entry.load()


@pytest.fixture(scope="module")
def records(golden_dir):
    piece = synth.read_fasta(os.path.join(golden_dir, "MEG3.fa"))[1][400:520]
    big = synth.planted_dna(sum(LENGTHS), SEED, piece, every=300, min_len=20, max_len=60)
    dnas, at = [], 0
    for n in LENGTHS:
        dnas.append(big[at:at + n])
        at += n
    return piece, dnas


_CASES = {}


def _case(mod, records, setting):
    """The restatement of every record under one setting, computed once and never changed."""
    if setting not in _CASES:
        piece, dnas = records
        p = mod.default_params(rule=setting[0], strand=setting[1])
        want = [expected_potential(piece, d, p) for d in dnas]
        for P, _ in want:
            P.setflags(write=False)
        _CASES[setting] = dict(setting=setting, p=p, piece=piece, dnas=dnas, P=[w[0] for w in want], per_enc=[w[1] for w in want])
    return _CASES[setting]


@pytest.fixture(scope="module", params=sorted(SETTINGS), ids=lambda s: f"r{s[0]}_t{s[1]}")
def case(request, mod, records):
    return _case(mod, records, request.param)


def _peaks(P, per_enc):
    """(4, 3) of (value, pos, enc): the first site of the class at min_value = the class's maximum is its peak"""
    pk = np.zeros((4, 3), dtype=np.int64)
    for c in range(4):
        top = int(P[c].max()) if P.shape[1] else 0
        rows = sites_from(P, per_enc, top) if top else []
        pk[c] = next(((r[3], r[4], r[5]) for r in rows if r[0] == c), (0, -1, -1))
    return pk


def test_the_class_tables_differ_and_leave_groups_empty(case):
    groups = [0] * 8
    for e in enabled_encodings(case["p"]):
        groups[enc_class(e) + 4 * (e & 1)] += 1
    assert groups == SETTINGS[case["setting"]]
    assert len({tuple(v) for v in SETTINGS.values()}) == 3
    # every class has rows of one direction at most, whatever the setting (the module's docstring)
    assert all(groups[c] == 0 or groups[4 + c] == 0 for c in range(4))


def test_the_case_is_not_vacuous(mod, records):
    case = _case(mod, records, (1, 0))
    assert case["p"].cutLength == 5000 and case["p"].overlapLength == 100
    held = 0
    for n, P in zip(LENGTHS, case["P"]):
        held += sum(int((P[:, k] > 0).sum()) for k in (2039, 2040, 4079, 4080) if k < n)
    print("non-zero (class, position) pairs at the slice edges:", held, "of", 4 * sum(k < n for n in LENGTHS for k in (2039, 2040, 4079, 4080)))
    assert held >= 20


def test_every_consumer_equals_the_restatement_and_the_others(mod, case):
    p, dnas, Ps, per_encs = case["p"], case["dnas"], case["P"], case["per_enc"]
    nonzero = np.concatenate([P[P > 0] for P in Ps])
    v = int(np.median(nonzero))          # about half of the non-zero positions reach it
    assert 1 < v < int(nonzero.max())
    e = mod.Engine(0)
    e.set_query(case["piece"])
    _, trk1, _ = e.scan_records_track(dnas, p, bin=1, records=False)
    _, trk7, pk7 = e.scan_records_track(dnas, p, bin=7, records=False)
    _, none, pk0 = e.scan_records_track(dnas, p, bin=0, records=False)
    _, sites = e.scan_sites(dnas, p, min_value=v, records=False)
    _, hist, _ = e.scan_hist(dnas, p)
    e.close()
    assert none is None
    from_tracks = np.zeros((4, 16384), dtype=np.int64)
    for r, (n, P, per_enc) in enumerate(zip(LENGTHS, Ps, per_encs)):
        what = f"record of {n} nt"
        t1 = trk1[r].array().astype(np.int64)
        _same(t1, P, what + ": track")
        _same(trk7[r].array(), bin_reduce(P, 7), what + ": track, bin 7")
        want_pk = _peaks(P, per_enc)
        _same(pk7[r], want_pk, what + ": peaks with bin 7")
        _same(pk0[r], want_pk, what + ": peaks only")
        _same(sites[r].array(), sites_from(P, per_enc, v), what + ": sites")
        _same(sites[r].array(), sites_from(t1, per_enc, v), what + ": sites against the track")
        from_tracks += bincount4(t1)
    assert np.array_equal(hist.array(), sum(bincount4(P) for P in Ps))
    assert np.array_equal(hist.array(), from_tracks)
    assert hist.positions == sum(LENGTHS) and not hist.pending
