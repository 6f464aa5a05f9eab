"""The joins of the batched read filter on host threads (gap2seq_amd/csrc/readfilter_gaps.cpp: filter_join_host), driven
through g2s_test_filter_join on rows and windows no BAM file of the suite produces, against a brute-force model written
from the definitions (tests/filter_join_model.py): exact equality of the return code and of both lists, on 1 and on 7
threads.  CPU only; tests/test_gpu_filter_join.py runs the same cases (tests/filter_join_cases.py) on the device joins."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import filter_join_cases as JC  # noqa: E402
import filter_join_model as M  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402


@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("case", JC.all_cases(), ids=lambda c: c["name"])
def test_host_joins_equal_the_model(case, threads):
    JC.check(P, case, device=-1, threads=threads)


def test_the_cap_is_reported_and_leaves_no_lists():
    hit = [c for c in JC.all_cases() if c["model"]["rc"] == M.ERR_NOMEM]
    assert len(hit) >= 3
    for c in hit:
        rc, l1, l2, msg = JC.run(P, c, device=-1, threads=3)
        assert rc == M.ERR_NOMEM and l1 == [] and l2 == [] and "G2S_FILTER_MAX_PAIRS" in msg


def test_a_device_that_cannot_run_the_kernels_is_an_error():
    """device >= 0 never runs the host joins in the device's place (no such device here: 2^20)"""
    c = JC.all_cases()[0]
    rc, l1, l2, msg = JC.run(P, c, device=1 << 20)
    assert rc == P.G2S_ERR_NO_DEVICE and l1 == [] and l2 == [] and "no usable gfx950 device" in msg


def test_the_host_switch_is_not_read(monkeypatch):
    monkeypatch.setenv("G2S_HOST_FILTER", "1")
    rc, _, _, _ = JC.run(P, JC.all_cases()[0], device=1 << 20)
    assert rc == P.G2S_ERR_NO_DEVICE


def test_small_output_capacities_are_answered_with_the_true_counts():
    """the hook allocates nothing for the caller: it returns both sizes and fills what fits"""
    import ctypes as C
    c = next(x for x in JC.all_cases() if x["name"] == "overlapping-flanks")
    m = c["model"]
    nr, n = len(c["pos"]), len(c["windows"]) // 3
    flat = [v for w in c["windows"] for v in w]
    l1, l2 = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    n1, n2 = C.c_uint64(0), C.c_uint64(0)
    rc = P.load_library().g2s_test_filter_join(
        -1, 2, nr, (C.c_int32 * nr)(*c["ref_id"]), (C.c_int32 * nr)(*c["pos"]), (C.c_int64 * nr)(*c["end"]),
        (C.c_uint32 * nr)(*c["flag"]), (C.c_uint64 * nr)(*c["h_own"]), (C.c_uint64 * nr)(*c["h_mate"]), c["max_span"],
        c["bits"], n, (C.c_int64 * len(flat))(*flat), c["max_pairs"], l1, 5, C.byref(n1), l2, 0, C.byref(n2))
    assert rc == 0 and n1.value == m["n1"] > 8 and n2.value == m["n2"] > 8
    assert [(x >> 32, x & 0xFFFFFFFF) for x in l1[:5]] == m["list1"][:5] and list(l1[5:]) == [0, 0, 0] and list(l2) == [0] * 8
