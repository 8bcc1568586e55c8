"""The frame of a call (csrc/engine.cpp: record_set_open / record_set_bounds, DESIGN.md "the frame of a call") seen through the Engine
methods: every record-set entry point refuses the same bad record sets with E_ARG and names the same record, and takes the whole
resident buffer for `dnas=None` where it takes it at all.  Nothing here provokes a fault: every bad set is refused before any
launch, the rest are scans of a 120 nt query and a 20 nt oligo over 900 nt.  GPU only.

A record past the resident buffer can be put only to the methods that take the records of the resident buffer as lengths or spans
(scan_records, scan_records_track, scan_regions, scan_regions_track): the others have no argument that could say it."""
import numpy as np
import pytest

import synth
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

RECS = [synth.random_dna(300, 11), synth.random_dna(290, 12), synth.random_dna(310, 13)]
WHOLE = b"".join(RECS)
QUERY = synth.random_dna(120, 7).replace(b"T", b"U")
OLIGO = QUERY[40:60]


@pytest.fixture(scope="module")
def mod():
    return entry.load()


@pytest.fixture(scope="module")
def eng(mod):
    e = mod.Engine(0)
    e.set_query(QUERY)
    return e


def _calls(mod, e):
    """name -> f(dnas): every record-set entry point on a record set given as `dnas`."""
    return {
        "scan_records": lambda d: e.scan_records(d),
        "scan_records_track": lambda d: e.scan_records_track(d, bin=1),
        "scan_tfo_profile": lambda d: e.scan_tfo_profile(d),
        "scan_sites": lambda d: e.scan_sites(d, min_value=15),
        "scan_sites_aligned": lambda d: e.scan_sites_aligned(d, min_value=15),
        "scan_hist": lambda d: e.scan_hist(d),
        "scan_oligos": lambda d: e.scan_oligos([OLIGO], d, min_value=15, track_bin=1),
        "scan_oligos_aligned": lambda d: e.scan_oligos_aligned([OLIGO], d, min_value=15),
        "scan_oligos_hist": lambda d: e.scan_oligos_hist([OLIGO], d),
        "score_variants": lambda d: e.score_variants([mod.Variant(1, "c", 100, ".", "A", "T")], d, flank=50),
    }


NAMES = sorted(_calls(None, None))
# the whole resident buffer as the one record: dnas=None alone says it
TAKE_NONE = ("scan_sites", "scan_sites_aligned", "scan_hist", "scan_oligos", "scan_oligos_aligned", "scan_oligos_hist", "score_variants")


def _refused(mod, f, *args):
    with pytest.raises(mod.FasimError) as ei:
        f(*args)
    assert ei.value.code == mod.E_ARG, str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("name", NAMES)
def test_no_record(mod, eng, name):
    assert "nrec = 0" in _refused(mod, _calls(mod, eng)[name], [])


@pytest.mark.parametrize("name", NAMES)
def test_empty_second_record(mod, eng, name):
    assert "record 1 is empty" in _refused(mod, _calls(mod, eng)[name], [RECS[0], b"", RECS[2]])


def test_nothing_resident(mod):
    """(an engine of its own: the module's gets its resident buffer in the tests below)"""
    e = mod.Engine(0)
    e.set_query(QUERY)
    calls = _calls(mod, e)
    for name in TAKE_NONE:
        assert "no resident DNA" in _refused(mod, calls[name], None), name
    assert "no resident DNA" in _refused(mod, lambda: e.scan_records(None, rec_lens=[300]))
    assert "no resident DNA" in _refused(mod, lambda: e.scan_records_track(None, rec_lens=[300], bin=1))
    assert "no resident DNA" in _refused(mod, lambda: e.scan_regions(None, [(0, 300)]))
    _refused(mod, calls["scan_tfo_profile"], None)      # (takes no resident buffer at all)
    e.close()


@pytest.fixture(scope="module")
def resident(eng):
    eng.load_dna(WHOLE)
    return eng


def test_record_past_the_resident_buffer(mod, resident):
    e = resident
    lens = [300, 290, 311]                               # one base more than the buffer holds
    spans = [(0, 300), (300, 590), (590, 901)]
    for f in (lambda: e.scan_records(None, rec_lens=lens), lambda: e.scan_records_track(None, rec_lens=lens, bin=1),
              lambda: e.scan_regions(None, spans), lambda: e.scan_regions_track(None, spans, bin=1)):
        text = _refused(mod, f)
        assert "record 2: offset 590, length 311 lies outside the DNA buffer (the resident buffer of fasim_load_dna)" in text


def _flat(x):
    """Every native object of a call's return value, in order, as comparable values."""
    if x is None:
        return []
    if isinstance(x, (list, tuple)):
        return [v for y in x for v in _flat(y)]
    if isinstance(x, np.ndarray):
        return [x.tolist()]
    if hasattr(x, "recs"):
        return [(x.recs, x.pool)]
    out = [x.array().tolist()]
    if hasattr(x, "cigars"):
        out.append(x.cigars())
    return out


@pytest.mark.parametrize("name", TAKE_NONE)
def test_none_is_the_resident_record(mod, resident, name):
    f = _calls(mod, resident)[name]
    got, want = _flat(f(None)), _flat(f([WHOLE]))
    assert got and got == want


def test_rec_lens_of_the_resident_buffer(mod, resident):
    e = resident
    lens = [len(r) for r in RECS]
    assert _flat(e.scan_records(None, rec_lens=lens)) == _flat(e.scan_records(RECS))
    assert _flat(e.scan_records_track(None, rec_lens=lens, bin=1)) == _flat(e.scan_records_track(RECS, bin=1))


def test_the_scans_find_something(mod, resident):
    """(so that the equalities above compare more than empty lists)"""
    _, sites = resident.scan_sites(None, min_value=15)
    assert len(sites[0]) > 0
    assert len(resident.scan_oligos([OLIGO], None, min_value=15)[0][0]) > 0
