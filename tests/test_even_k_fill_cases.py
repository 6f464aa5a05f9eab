"""The designed even-k gap lists (tests/even_k_fill_cases.py) under the oracle alone: every class must have a gap that
the oracle fills, without a Q7 flag, through the planted palindrome — otherwise the GPU tests built on these lists
(tests/test_gpu_even_k_fill.py) would compare nothing next to a palindrome."""
import pytest

import even_k_fill_cases as E
import pyref


def oracle_outcomes(oracle, reads, gaps, k, allp, seed=5):
    og = oracle.OracleGraph(reads, k, 1)
    rng = oracle.OracleRng(seed)
    try:
        out = []
        for g in gaps:
            o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], E.D_ERR, g["lmf"], g["rmf"], False, allp)
            out.append((o.count, o.info.q7, o.fill, o.info.draws))
        return out
    finally:
        rng.free()
        og.free()


@pytest.mark.parametrize("allp", [True, False])
@pytest.mark.parametrize("k", E.K)
def test_every_class_has_a_gap_filled_through_its_palindrome(oracle, k, allp):
    reads, gaps = E.build(k)
    assert {g["cls"] for g in gaps} == set(E.CLASSES + "g")
    for g in gaps:
        assert len(g["pal"]) == k and g["pal"] == pyref.revcomp(g["pal"])
    good = E.class_condition(gaps, oracle_outcomes(oracle, reads, gaps, k, allp))
    assert all(good[c] for c in E.CLASSES)


def test_the_padded_list_is_just_over_the_resident_threshold(oracle):
    reads, gaps = E.padded(32)
    assert 256 < len(gaps) <= 272 and gaps[:len(E.build(32)[1])] == E.build(32)[1]
    out = oracle_outcomes(oracle, reads, gaps, 32, True)
    E.class_condition(gaps, out)
    assert sum(1 for g, o in zip(gaps, out) if g["cls"] is None and o[0] > 0) > 150
