"""Pass B of the batched read filter without a GPU: the host walk (g2s_test_bam_text, device -1) on the designed files of
tests/bam_text_cases.py against a pure-Python decode of the same bytes — which pins the authority the kernels are
compared with in tests/test_gpu_bam_text.py — and the switches of one-pass mode (g2s_filter_set_one_pass,
G2S_FILTER_ONE_PASS), which without a device must change nothing but the reason the hook reports."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_text_cases as TC  # noqa: E402
import bam_walk_cases as WC  # noqa: E402
import filter_gap_cases as FC  # noqa: E402

G2S_OK, G2S_ERR_ARG = 0, -1
NOT_ASKED, NO_DEVICE_ROWS = 1, 2
FILES = (TC.designed(),) + TC.small_files()


@pytest.fixture
def mode(product, monkeypatch):
    """every test starts and ends in the initial state: the mode follows the environment, which says nothing"""
    monkeypatch.delenv("G2S_FILTER_ONE_PASS", raising=False)
    product.filter_set_one_pass(-1)
    yield product
    product.filter_set_one_pass(-1)


def test_the_designed_file_holds_what_it_is_for():
    recs = TC.records(TC.designed().raw)
    assert {len(c) for _, _, c in recs} >= set(TC.LENGTHS)
    for n in TC.LENGTHS:
        assert {f & TC.REVERSE for _, f, c in recs if len(c) == n} == {0, TC.REVERSE}, n
    assert sum(1 for _, _, c in recs if sorted(c) == list(range(16))) == 2
    assert {len(nm) for nm, _, _ in recs} >= {0, 1, 254}
    assert (b"ab", TC.READ1, [8, 4, 2]) in recs
    assert {f & (TC.READ1 | TC.READ2) for _, f, _ in recs} == {0, TC.READ1, TC.READ2, TC.READ1 | TC.READ2}
    assert [len(TC.records(c.raw)) for c in TC.small_files()] == [0, 1]
    assert TC.bases_of(0, range(16)) == b"NACNGNNNTNNNNNNN" and TC.bases_of(16, range(16)) == b"NNNNNNNANNNCNGTN"


@pytest.mark.parametrize("case", FILES, ids=lambda c: c.name)
def test_host_walk_equals_python_decode(product, case):
    n = len(TC.records(case.raw))
    for what, rows in TC.selections(n):
        for names, fasta in ((True, False), (False, False), (False, True)):
            rc, got, msg = product.bam_text(case.data, rows, device=-1, names=names, fasta=fasta)
            assert rc == G2S_OK, (what, msg)
            assert got == TC.expected(case.raw, rows, names, fasta), (what, names, fasta)


def test_host_walk_on_the_cut_files_equals_python_decode(product, monkeypatch):
    assert len(TC.window_cases()) > 2 * len(WC.designed_cases()) - 4
    for case in TC.window_cases():
        if case.chunk:
            monkeypatch.setenv("G2S_BAM_CHUNK", str(case.chunk))
        else:
            monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)
        rows = list(range(len(TC.records(case.raw))))
        for fasta in (False, True):
            rc, got, msg = product.bam_text(case.data, rows, device=-1, names=True, fasta=fasta)
            assert rc == G2S_OK, (case.name, msg)
            assert got == TC.expected(case.raw, rows, True, fasta), case.name


def test_a_row_beyond_the_file_is_an_argument_error(product):
    case = TC.designed()
    rc, got, msg = product.bam_text(case.data, [len(TC.records(case.raw))], device=-1)
    assert (rc, got) == (G2S_ERR_ARG, None) and "beyond" in msg


def test_the_setter_returns_the_previous_mode(mode):
    assert mode.filter_set_one_pass(1) == -1
    assert mode.filter_set_one_pass(0) == 1
    assert mode.filter_set_one_pass(-1) == 0
    assert mode.filter_set_one_pass(7) == -1   # (anything positive asks, anything negative follows the environment)
    assert mode.filter_set_one_pass(-5) == 1
    assert mode.filter_set_one_pass(-1) == -1


def _calls(P, bam, gaps):
    texts, stats, un = P.filter_reads_gaps(bam, 300, 20, gaps, device=-1, unmapped=True)
    hook = P.last_filter_text()
    pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    got = (texts, un, [pool.fasta(i) for i in range(len(gaps))], pool.unmapped_fasta(), pool.n_reads, pool.total,
           stats["file_passes"], pool.stats["file_passes"], stats["on_device"])
    pool.free()
    return got, hook, P.last_filter_text()


def test_without_a_device_asking_changes_nothing(mode):
    bam, _, gaps = FC.simulated(7)
    plain, hook, hook_pool = _calls(mode, bam, gaps)
    assert (hook["one_pass"], hook["reason"], hook["resident_bytes"]) == (0, NOT_ASKED, 0) and hook_pool == hook
    mode.filter_set_one_pass(1)
    asked, hook, hook_pool = _calls(mode, bam, gaps)
    assert (hook["one_pass"], hook["reason"], hook["reads"], hook["bytes"], hook["resident_bytes"]) == (0, NO_DEVICE_ROWS, 0, 0, 0)
    assert hook_pool == hook
    assert asked == plain
    assert plain[6] == plain[7] == 2 and plain[8] == 0
    assert sum(x[3] for x in plain[0]) > 0


def test_the_environment_asks_and_the_setter_overrides_it(mode, monkeypatch):
    bam, _, gaps = FC.simulated(7)

    def reason():
        mode.filter_reads_gaps(bam, 300, 20, gaps[:2], device=-1)
        return mode.last_filter_text()["reason"]

    assert reason() == NOT_ASKED                     # neither set: off
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "1")   # read per call
    assert reason() == NO_DEVICE_ROWS
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "0")
    assert reason() == NOT_ASKED
    mode.filter_set_one_pass(1)                      # the setter goes first, either way
    assert reason() == NO_DEVICE_ROWS
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "1")
    mode.filter_set_one_pass(0)
    assert reason() == NOT_ASKED
    mode.filter_set_one_pass(-1)
    assert reason() == NO_DEVICE_ROWS
