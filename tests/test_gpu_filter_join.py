"""The joins of the batched read filter on the MI355X (gap2seq_amd/csrc/readfilter_gpu.hip: k_bits, k_gap, k_mates and
the rocPRIM sorts, scans and unique between them), driven through g2s_test_filter_join with device 0 on the cases of
tests/filter_join_cases.py, against the brute-force model of tests/filter_join_model.py: exact equality of the return
code and of both lists.  The cases reach what no BAM file of the suite does: a populated right-hand window, a longest
span far beyond the read length, (bit, gap) keys beyond 2^63, the clamps of the index key, windows of exactly 63 / 64 /
65 / 128 rows, 65 537 gaps, the empty filter with a non-empty list 2, and the three checks of the pair cap.  The hook
never runs the host joins in the device's place, so nothing here can pass without the kernels.

Cost on one MI355X: this file alone, 79 tests in 7 s (pytest's own figure, the model's runs during collection
included); the two one-row cases of degenerate() came later and make it 81.  The whole `-m gpu` suite with it and with the ten libraries added to tests/filter_gap_cases.py: 455 tests
in 388 s; none of the added tests is among that run's 60 slowest (the 60th took 0.86 s), so the suite without them
took between 372 and 381 s on the same machine."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import filter_join_cases as JC  # noqa: E402
import filter_join_model as M  # noqa: E402
from test_gpu_parity import _gaps  # noqa: E402
from test_gpu_resident import _key  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", JC.all_cases(), ids=lambda c: c["name"])
def test_device_joins_equal_the_model(product, case):
    JC.check(product, case, device=0)


def test_sweep_device_equals_host(product):
    """the sweep once more, device against host: with the model's verdicts this names the side that differs"""
    for c in JC.sweep_cases():
        assert JC.run(product, c, device=0)[:3] == JC.run(product, c, device=-1, threads=4)[:3], c["name"]


def test_the_cap_is_checked_on_the_device_at_all_three_counts(product):
    hit = [c for c in JC.all_cases() if c["model"]["rc"] == M.ERR_NOMEM]
    assert len(hit) >= 3
    for c in hit:
        rc, l1, l2, msg = JC.run(product, c, device=0)
        assert rc == M.ERR_NOMEM and l1 == [] and l2 == [] and "G2S_FILTER_MAX_PAIRS" in msg, c["name"]


def test_twenty_calls_in_one_process_leave_no_state(product):
    names = ("high-bits", "no-filter-rows", "wave-edges", "cap-nb+n1-1", "gaps-257", "no-rows", "dense-bits1", "cap-exact",
             "coordinates", "no-flank-rows")
    by_name = {c["name"]: c for c in JC.all_cases()}
    for i in range(20):
        JC.check(product, by_name[names[i % len(names)]], device=0)


def test_a_join_beside_a_live_fill_session(product):
    """The joins use the null stream and hipDeviceSynchronize: a call made while a fill session is alive on the same
    device changes neither its own answer nor the session's next list."""
    k, e = 31, 20
    seqs = cases.toy_genome(977, 30000, k, repeats=6, tandem=2, snp_every=500)
    gaps = cases.cut_gaps(977, seqs[0], k, 10, 24, 20, 200, e)
    c = next(x for x in JC.all_cases() if x["name"] == "sweep-00-small")
    pg = product.Graph.from_seqs(seqs, k, 1)
    sess = product.Session(pg, 0, d_err=e, randseed=5)
    try:
        before = [_key(r) for r in sess.fill_batch(_gaps(product, gaps))]
        sess.srand(5)
        JC.check(product, c, device=0)
        after = [_key(r) for r in sess.fill_batch(_gaps(product, gaps))]
        JC.check(product, c, device=0)
    finally:
        sess.destroy()
        pg.free()
    assert after == before and any(r[0] > 0 for r in before)
