"""The host graph build at even k (gap2seq_amd/csrc/dbg.cpp) against pyref.Graph on the designed reads of
tests/even_k_cases.py: palindromic k-mers at the centre of a hairpin, in periodic reads, in the middle and at the end
of a non-branching path, next to a branch, isolated, and on a cycle.  The device build (tests/test_gpu_even_k_build.py)
is held to this builder, so this pins the authority.  No GPU: G2S_HOST_BUILD=1 keeps the build on host threads."""
import pytest

import even_k_cases as EK

KS = [2, 4, 12, 30, 32, 64, 96, 126]


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_host_build_of_the_designed_reads_is_pyrefs_graph(product, monkeypatch, k, solid):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    reads, designed = EK.designed_reads(k, solid)
    g = product.Graph.from_seqs(reads, k, solid)
    try:
        EK.assert_graph_is_pyrefs(g, reads, k, solid, designed)
    finally:
        g.free()


@pytest.mark.parametrize("k", [30, 64])
def test_host_graph_with_palindromes_survives_save_and_load(product, monkeypatch, tmp_path, k):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    reads, designed = EK.designed_reads(k, 1)
    g = product.Graph.from_seqs(reads, k, 1)
    try:
        path = str(tmp_path / "g.bin")
        g.save(path)
        h = product.Graph.load(path)
        try:
            assert EK.graph_map(h) == EK.graph_map(g) and h.num_unitigs == g.num_unitigs and h.validate() == (0, "")
        finally:
            h.free()
    finally:
        g.free()
