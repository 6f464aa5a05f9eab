"""The store route of the batched read filter's one-pass mode (gap2seq_amd/csrc/bam_store.h), the part that needs no GPU: the
host model of the store (g2s_test_bam_store, device -1) against a Python compaction written from the format
(tests/bam_store_cases.py) — which pins what the kernels are compared with in tests/test_gpu_filter_store.py —, the plan
of the two capacities (g2s_test_filter_store_plan) against the rule restated, and the switch without a device."""
import functools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_store_cases as SC  # noqa: E402
import bam_text_cases as TC  # noqa: E402
import bam_walk_cases as WC  # noqa: E402
import filter_gap_cases as FC  # noqa: E402

G2S_OK = 0
NO_DEVICE_ROWS = 2
FILES = (TC.designed(),) + TC.small_files() + tuple(WC.field_cases())
FORMS = ((True, False), (False, False), (False, True))   # (names, fasta)
SWITCHES = ("G2S_FILTER_ONE_PASS", "G2S_FILTER_RESIDENT_CAP", "G2S_FILTER_STORE", "G2S_FILTER_STORE_SAMPLE", "G2S_BAM_CHUNK")


@pytest.fixture
def P(product, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    product.filter_set_one_pass(-1)
    yield product
    product.filter_set_one_pass(-1)


# ---- the host model against the format

@pytest.mark.parametrize("case", FILES, ids=lambda c: c.name)
def test_host_model_equals_python_compaction(P, case):
    rc, got, msg = P.bam_store(case.data, device=-1)
    assert rc == G2S_OK, msg
    store, offs = SC.compact(case.raw)
    assert got[1] == offs
    assert got[0] == store
    src = SC.source_records(case.raw)
    assert len(offs) == len(src) and len(store) == sum(SC.stored_bytes(ln, ls) for _, _, ln, _, ls in src)
    # a stored record is never longer than its source, and the store is a BAM record stream pass B reads the same way
    assert all(SC.stored_bytes(ln, ls) <= 4 + bs for _, bs, ln, _, ls in src)
    as_stream = WC.header() + store
    assert [o - WC.FIRST for o, _, _, _, _ in SC.source_records(as_stream)] == offs
    assert all(nc == 0 and bs == SC.stored_bytes(ln, ls) - 4 for _, bs, ln, nc, ls in SC.source_records(as_stream))
    for what, rows in TC.selections(len(src)):
        for names, fasta in FORMS:
            assert TC.expected(as_stream, rows, names, fasta) == TC.expected(case.raw, rows, names, fasta), (what, names, fasta)


def test_the_files_hold_what_the_store_is_checked_on():
    src = SC.source_records(TC.designed().raw)
    assert {ln for _, _, ln, _, _ in src} >= {2, 6, 255} and {ls for _, _, _, _, ls in src} >= {0, 1, 2, 3, 3001}
    assert 1 in {ln for _, _, ln, _, _ in SC.source_records(WC.field_cases()[0].raw)}   # (a name that is its NUL alone)
    assert any(nc > 1 for c in WC.field_cases() for _, _, _, nc, _ in SC.source_records(c.raw))
    fields = WC.field_cases()[0].raw
    assert b"NMC\x03XZhello" in fields and b"NMC\x03XZhello" not in SC.compact(fields)[0]   # (tags are not kept)
    store, _ = SC.compact(TC.designed().raw)
    assert len(store) < len(TC.designed().raw) - WC.FIRST


# ---- the plan

def _plan(P, data):
    rc, got, msg = P.filter_store_plan(data)
    assert rc == G2S_OK, msg
    return got


@functools.lru_cache(maxsize=None)
def _library():
    """the 6 080-record library of tests/test_gpu_bam_text.py"""
    import bamwriter as BW
    refs, recs, _ = BW.simulate_library(43, n_scaffolds=2, scaffold_len=12000, gap=(6000, 250), pairs=1500, unmapped_pairs=40)
    return BW.bam_bytes(refs, recs, block=5000), len(recs)


def test_plan_of_a_file_that_is_all_sample(P):
    for case in (TC.designed(),) + tuple(WC.field_cases()):
        got = _plan(P, case.data)
        src = SC.source_records(case.raw)
        Pb = len(case.raw) - WC.FIRST
        assert (got["sample_records"], got["sample_bytes"]) == (len(src), Pb)
        assert got["sample_stored"] == len(SC.compact(case.raw)[0])
        assert got == SC.plan_of(case.raw)
        assert got["rows_cap"] <= Pb // 36 + 1 and got["store_cap"] <= Pb
        assert got["need"] == 52 * (got["rows_cap"] + 1) + got["store_cap"]
        # the margin holds what the file holds when the whole file is the sample
        assert got["rows_cap"] >= len(src) and got["store_cap"] >= got["sample_stored"]


def test_the_two_formulas():
    assert SC.plan(1000000, 100, 10000, 4000) == dict(rows_cap=12500 + 64, store_cap=500000 + 4096, need=52 * 12565 + 504096)
    assert SC.plan(1000000, 3, 1000, 7)["rows_cap"] == 3750 + 64          # 1.25 * 3 / 1000 * 10^6
    assert SC.plan(999, 1, 7, 7) == dict(rows_cap=999 // 36 + 1, store_cap=999, need=52 * 29 + 999)   # (the worst case bounds both)
    assert SC.plan(10 ** 6, 1, 3, 1)["store_cap"] == -(-5 * 10 ** 6 // 12) + 4096                       # (the ceiling)
    assert SC.plan(10 ** 6, 0, 0, 0) == dict(rows_cap=64, store_cap=4096, need=52 * 65 + 4096)


def test_plan_of_a_file_without_records(P):
    got = _plan(P, TC.small_files()[0].data)
    assert got == dict(sample_records=0, sample_bytes=0, sample_stored=0, rows_cap=1, store_cap=0, need=104)


def test_the_sample_switch_and_a_boundary_inside_a_record(P, monkeypatch):
    bam, n = _library()
    rc, raw, _, _ = P.bgzf_inflate(bam, -1)
    assert rc == G2S_OK
    first = len(raw) - sum(4 + bs for _, bs, _, _, _ in _records(raw))
    whole = _plan(P, bam)   # (smaller than 1 MiB: all sample)
    assert (whole["sample_records"], whole["sample_bytes"]) == (n, len(raw) - first)
    src = _records(raw)
    for sample in (1, 36, 4 + src[0][1], 4 + src[0][1] + 1, 16384, 100000):
        monkeypatch.setenv("G2S_FILTER_STORE_SAMPLE", str(sample))
        got = _plan(P, bam)
        taken = [s for s in src if s[0] < first + sample]
        assert taken and taken[-1][0] + 4 + taken[-1][1] >= first + sample       # (the last one reaches the boundary or beyond it)
        assert got["sample_records"] == len(taken)
        assert got["sample_bytes"] == sum(4 + bs for _, bs, _, _, _ in taken)     # (it is counted whole)
        assert got["sample_stored"] == sum(SC.stored_bytes(ln, ls) for _, _, ln, _, ls in taken)
        want = SC.plan(len(raw) - first, got["sample_records"], got["sample_bytes"], got["sample_stored"])
        assert {k: got[k] for k in want} == want
    assert _plan(P, bam)["sample_bytes"] > 100000
    monkeypatch.setenv("G2S_FILTER_STORE_SAMPLE", "0")   # (nothing sensible: the default)
    assert _plan(P, bam) == whole


def _records(raw):
    """source_records for a stream with any header"""
    import struct
    l_text, = struct.unpack_from("<i", raw, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, o)
    o += 4
    for _ in range(n_ref):
        ln, = struct.unpack_from("<i", raw, o)
        o += 8 + ln
    out = []
    while o < len(raw):
        bs, = struct.unpack_from("<I", raw, o)
        _, _, l_name, _, _, n_cigar, _, l_seq = struct.unpack_from("<iiBBHHHi", raw, o + 4)
        out.append((o, bs, l_name, n_cigar, l_seq))
        o += 4 + bs
    return out


def test_the_library_of_the_end_to_end_test(P):
    """747 241 inflated bytes; the whole stream needs raw + 52 (raw // 36 + 1) = 1 826 605 bytes; the store route's margin
    on what the file holds is 1.25 (52 r + c) = 911 850 bytes, and with the additive terms its need is 919 326"""
    bam, n = _library()
    rc, raw, _, _ = P.bgzf_inflate(bam, -1)
    assert rc == G2S_OK and (n, len(raw)) == (6080, 747241)
    assert len(raw) + 52 * (len(raw) // 36 + 1) == 1826605
    got = _plan(P, bam)
    assert (got["sample_records"], got["sample_stored"]) == (6080, 413320)
    assert 5 * (52 * 6080 + 413320) // 4 == 911850
    assert got["need"] == 911850 + 52 * (64 + 1) + 4096 == 919326
    assert got["rows_cap"] >= n and got["store_cap"] >= sum(SC.stored_bytes(ln, ls) for _, _, ln, _, ls in _records(raw))


def test_each_overflow_file_overflows_its_capacity_alone(P, monkeypatch):
    monkeypatch.setenv("G2S_FILTER_STORE_SAMPLE", str(SC.OVERFLOW_SAMPLE))
    for case, rows_over, store_over in ((SC.rows_overflow(), True, False), (SC.store_overflow(), False, True)):
        got = _plan(P, case.data)
        assert got == SC.plan_of(case.raw, SC.OVERFLOW_SAMPLE)
        assert 50 < got["sample_records"] < 60
        store, offs = SC.compact(case.raw)
        assert (len(offs) > got["rows_cap"]) == rows_over, case.name
        assert (len(store) > got["store_cap"]) == store_over, case.name
    assert _plan(P, SC.rows_overflow().data)["store_cap"] == len(SC.rows_overflow().raw) - WC.FIRST   # (it cannot overflow)
    # without the switch either file is all sample, and nothing overflows
    monkeypatch.delenv("G2S_FILTER_STORE_SAMPLE")
    for case in (SC.rows_overflow(), SC.store_overflow()):
        got = _plan(P, case.data)
        store, offs = SC.compact(case.raw)
        assert len(offs) <= got["rows_cap"] and len(store) <= got["store_cap"]


# ---- without a device

def test_without_a_device_the_switch_changes_nothing(P, monkeypatch):
    bam, _, gaps = FC.simulated(7)
    plain, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=-1)
    monkeypatch.setenv("G2S_FILTER_STORE", "1")
    P.filter_set_one_pass(1)
    asked, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=-1)
    hook, store = P.last_filter_text(), P.last_filter_store()
    assert stats["file_passes"] == 2 and (hook["one_pass"], hook["reason"], hook["resident_bytes"]) == (0, NO_DEVICE_ROWS, 0)
    assert store == dict(used=0, overflow=0, records=0, store_bytes=0, store_cap=0, rows_cap=0, device_bytes=0)
    assert asked == plain and sum(x[3] for x in plain) > 0
    pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    assert pool.stats["file_passes"] == 2 and P.last_filter_text()["reason"] == NO_DEVICE_ROWS
    pool.free()
