"""The decoder of the device inflate (gap2seq_amd/csrc/inflate_core.h) compiled for the host, against zlib, without a
GPU: every designed and corrupt member of tests/inflate_cases.py through g2s_test_bgzf_inflate with device -2 (the
kernel's decoder and its CRC by slices) and -1 (zlib, the product's host path), and a seeded corpus of 200 members."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import inflate_cases as IC  # noqa: E402

G2S_OK, G2S_ERR_IO = 0, -2


def test_the_designs_are_what_they_claim():
    IC.self_check()
    names = [c[0] for c in IC.valid_cases()] + [c[0] for c in IC.corrupt_cases()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", IC.valid_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("eof", [True, False], ids=["eof", "no_eof"])
def test_valid_member(product, case, eof):
    _, m, payload = case
    data = m + (IC.EOF if eof else b"")
    for device in (-2, -1):
        rc, got, bad, msg = product.bgzf_inflate(data, device)
        assert rc == G2S_OK, (device, msg)
        assert got == payload, device
        assert bad == -1


def test_all_valid_members_as_one_file(product):
    for eof in (True, False):
        data, payload = IC.valid_file(eof)
        for device in (-2, -1):
            rc, got, _, msg = product.bgzf_inflate(data, device)
            assert rc == G2S_OK, msg
            assert got == payload


@pytest.mark.parametrize("case", IC.corrupt_cases(), ids=lambda c: c[0])
def test_corrupt_member(product, case):
    _, m = case
    seen = []
    for data, where in ((m + IC.EOF, 0), (IC.corrupt_file(m), 1)):
        for device in (-2, -1):
            rc, got, bad, msg = product.bgzf_inflate(data, device)
            assert rc == G2S_ERR_IO, device
            assert bad == where, device
            assert msg == "corrupt BGZF block %d" % where
            seen.append((rc, bad, msg))
    assert seen[0] == seen[1] and seen[2] == seen[3]
    # nothing is left behind for the file that follows
    data, payload = IC.good_file_after()
    assert product.bgzf_inflate(data, -2)[:2] == (G2S_OK, payload)


def test_windows_smaller_than_the_file(product, monkeypatch):
    data, payload = IC.valid_file()
    monkeypatch.setenv("G2S_BAM_CHUNK", "70000")
    for device in (-2, -1):
        rc, got, _, msg = product.bgzf_inflate(data, device)
        assert rc == G2S_OK, msg
        assert got == payload


def test_random_corpus(product):
    data, payload = IC.random_corpus()
    assert len(IC.split_members(data)) == 201
    want = product.bgzf_inflate(data, -1)
    assert want[0] == G2S_OK and want[1] == payload
    assert product.bgzf_inflate(data, -2) == want
