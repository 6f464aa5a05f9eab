"""Pass A of the batched read filter without a GPU: csrc/name_hash.h against std::hash<std::string>, and the host walk
(g2s_test_bam_rows, device -1) on the designed files of tests/bam_walk_cases.py against a pure-Python parse of the same
bytes — which pins the fixtures the kernels are compared with in tests/test_gpu_bam_rows.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_walk_cases as WC  # noqa: E402

G2S_OK, G2S_ERR_IO = 0, -2
ALL = WC.designed_cases() + WC.handed_over_cases()


def test_name_hash_is_std_hash(product):
    names = WC.hash_names()
    assert len(names) > 580
    for name in names:
        for which in (1, 2):
            std, own = product.name_hash(name, which)
            assert std == own, (name, which)
            assert own == WC.std_hash(name.split(b"\0")[0] + (b"/1" if which == 1 else b"/2")), (name, which)


def test_name_hash_hook_checks_its_arguments(product):
    with pytest.raises(product.G2SError):
        product.name_hash(b"x", 3)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_host_walk_equals_python_parse(product, case):
    rc, rows, msg = product.bam_rows(case.data, -1)
    assert rc == G2S_OK, msg
    want = WC.parse(case.raw)
    assert rows == want
    hook = product.last_filter_rows()
    assert (hook["on_device"], hook["anomaly"], hook["records"]) == (0, 0, want["total"])


def test_designed_files_hold_what_they_are_named_for():
    by = {c.name: c for c in ALL}
    assert WC.parse(by["records_4097"].raw)["total"] == 4097
    assert WC.parse(by["records_0"].raw)["total"] == 0
    f = WC.parse(by["fields"].raw)
    assert f["end"][0] == f["pos"][0] + 1 and f["end"][1] == f["pos"][1] + 1  # no CIGAR; S/I/H/P only
    assert f["end"][2] == f["pos"][2] + 10 + 2 + 300 + 4 + 5                   # M D N = X
    assert f["end"][3] == f["pos"][3] + 1                                     # unmapped: its CIGAR does not count
    assert f["h_own"][7] == f["h_mate"][8]                                    # "inner\0nul_x" is "inner"
    m = WC.parse(by["maxima_by_a_record_without_reference"].raw)
    assert m["read_length"] == 300 and m["max_span"] == 20
    assert WC.parse(by["maxima_by_the_first_record"].raw)["max_span"] == 500
    assert WC.parse(by["maxima_by_the_last_record"].raw)["read_length"] == 120


@pytest.mark.parametrize("case", WC.error_cases(), ids=lambda c: c[0])
def test_host_walk_rejects_the_broken_files(product, monkeypatch, case):
    _, data, chunk, text = case
    if chunk:
        monkeypatch.setenv("G2S_BAM_CHUNK", str(chunk))
    rc, rows, msg = product.bam_rows(data, -1)
    assert (rc, rows, msg) == (G2S_ERR_IO, None, text)
