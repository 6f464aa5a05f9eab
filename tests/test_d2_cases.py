"""The designed cyclic closures of tests/d2_cases.py on the CPU, before tests/test_gpu_d2_designed.py takes them to the
device: a design that does not have the component structure it was written for fails here, where it is written.

Every design against the oracle's subgraph statistics (nontrivial strong components, their size, the extra conditions
of its table row), against the string restatement oracle/pyref.py (count, fuz, fill, draws and all six statistics) and,
through test_seg_model's chain — the segment tier's model, g2s_test_seg_expand, g2s_test_post_closure — against the
host version of phase D2 (post.cpp).  The model takes every design: none is left out of that leg.  The pyref leg
leaves out the designs marked slow (loop-in-component: 14 s of Python dicts for a count that saturates)."""
import pytest

import cases
import d2_cases as DC
import pyref
from test_seg_model import _ladder_model, check_config

K = DC.K
_ORACLE = {}


def _oracle_fill(oracle, name):
    """The oracle's result for one design, alone on its own graph (computed once)."""
    if name not in _ORACLE:
        d = DC.design(name)
        g = d["gap"]
        og = oracle.OracleGraph(d["seqs"], K, 1)
        rng = oracle.OracleRng(5)
        try:
            _ORACLE[name] = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], d["d_err"], g["lmf"], g["rmf"])
        finally:
            rng.free()
            og.free()
    return _ORACLE[name]


def test_the_table_has_fifteen_designs_on_four_lists():
    assert len(DC.NAMES) == 15 and DC.D_ERRS == [40, 150, 200, 300]  # (a list each: the comparison takes -dist-error per list)
    assert [n for n in DC.NAMES if DC.DESIGNS[n][3].get("csize") is None] == ["figure-8"]
    for n in DC.NAMES:
        g = DC.design(n)["gap"]
        assert (g["lmf"], g["rmf"]) == (3, 3) and len(g["left"]) == len(g["right"]) == K + 3
        assert g["true_len"] < 3500


def test_strand_clean_allows_repeats_and_nothing_else():
    s = cases.random_dna(cases.SplitMix(77), 120)
    rc = s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    assert DC.strand_clean([s * 3]) and not cases.clean_haplotypes([s * 3], K)  # (a repeat: fine here)
    assert not DC.strand_clean([s, "ACGT" + rc[40:40 + K] + "ACGT"])  # a k-mer meets its reverse complement
    assert not DC.strand_clean([s + rc[:K]])
    pal = s[:6] + rc[-6:]
    assert not DC.strand_clean(["CC" + pal + "CC"], 12) and DC.strand_clean(["CC" + pal + "CC"], 13)  # its own reverse complement


@pytest.mark.parametrize("name", DC.NAMES)
def test_design_has_its_designed_components(oracle, name):
    d = DC.design(name)
    want = d["want"]
    o = _oracle_fill(oracle, name)
    assert not o.info.q7
    assert o.phase_d and o.count > 0
    vertices, edges, ncomp, csize = o.substats[:4]
    assert ncomp == want["ncomp"]
    if want["csize"] is not None:
        assert csize == want["csize"]
    else:
        assert csize > 0  # (figure-8, recorded: 157)
    if "count" in want:
        assert o.count == want["count"]
    if want.get("loop"):
        assert edges == vertices  # a path from source to sink has one edge less than vertices: the loop is the one more
    # both verdicts in one fill: a kernel that calls every run safe, or none, cannot pass
    assert any(c.isupper() for c in o.fill) and any(c.islower() for c in o.fill)


@pytest.mark.parametrize("name", [n for n in DC.NAMES if not DC.DESIGNS[n][3].get("slow")])
def test_design_equals_the_python_restatement(oracle, name):
    d = DC.design(name)
    g = d["gap"]
    o = _oracle_fill(oracle, name)
    pi = pyref.Info()
    c2, lf2, rf2, fill2, sub2 = pyref.fill_gap(pyref.Graph(d["seqs"], K, 1), pyref.GlibcRand(5), g["left"], g["right"],
                                               g["gap_len"], d["d_err"], g["lmf"], g["rmf"], False, True, True, pi)
    assert (o.count, o.left_fuz, o.right_fuz) == (c2, lf2, rf2)
    assert (o.info.phaseC_count, o.lengths, o.info.draws, o.info.q7) == (pi.phaseC_count, pi.lengths, pi.draws, pi.q7)
    assert o.fill == pyref.fill_string(fill2, g["lmf"] - lf2)
    assert o.substats == [sub2[x] for x in ("vertices", "edges", "nontrivial", "size_nontrivial", "vertices_final",
                                            "edges_final")]


@pytest.mark.parametrize("name", DC.NAMES)
def test_design_through_the_model_and_the_hosts_phase_d(product, oracle, name):
    """test_seg_model's chain on the design: the model's states, counts and closure are the oracle's, and the host's
    phase D on that closure (post.cpp: per-state records, and the analysis on runs) gives the oracle's count, fuz,
    draws, fill and statistics.  With -best-only too (the closure of the first path lengths found)."""
    d = DC.design(name)
    assert check_config(product, oracle, d["seqs"], K, [d["gap"]], d["d_err"]) == (1, 0)
    assert check_config(product, oracle, d["seqs"], K, [d["gap"]], d["d_err"], allp=False) == (1, 0)


@pytest.mark.parametrize("name", DC.NAMES)
def test_design_has_the_closure_segments_its_row_says(product, oracle, name):
    """`ncl`: the closure's segments, by which phase D2 on the device chooses its instantiation (g2s_d2_small takes
    256); the model's count is the oracle's."""
    d = DC.design(name)
    m, _, o = _ladder_model(product, oracle, d, d["d_err"])
    assert not m.q7 and m.c_count == o.info.phaseC_count and m.lengths == o.lengths
    assert len(m.compact) == d["want"]["ncl"]


@pytest.mark.parametrize("d_err", DC.D_ERRS)
def test_designs_of_one_list_share_no_kmer(oracle, d_err):
    """tests/test_gpu_d2_designed.py runs the designs of one -dist-error as one list on one graph, among ordinary gaps:
    no design's k-mer is another's or the plain genome's, on either strand, so every closure is the one checked above."""
    seqs, gaps, idx, names = DC.design_list(d_err, pad=100)
    assert len(gaps) == 100 + len(names) and DC.strand_clean(seqs)
    assert [gaps[i] for i in idx] == [DC.design(n)["gap"] for n in names]
    seen = set()
    for n in names + ["the plain genome"]:
        mine = DC.kmers(DC.design(n)["seqs"] if n in DC.DESIGNS else seqs[-1:])
        assert not mine & seen, n
        seen |= mine
    og = oracle.OracleGraph(seqs, K, 1)
    rng = oracle.OracleRng(5)
    try:
        for n in names:
            g = DC.design(n)["gap"]
            o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], d_err, g["lmf"], g["rmf"])
            alone = _oracle_fill(oracle, n)
            assert (o.count, o.substats, o.lengths, len(o.fill)) == (alone.count, alone.substats, alone.lengths, len(alone.fill)), n
    finally:
        rng.free()
        og.free()
