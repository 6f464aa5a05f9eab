"""A single graph bounded to its gap list's reach, on the host (g2s_graph_build_seqs_reach, gap2seq_amd/csrc/dbg.cpp:
reach_filter_host): the kept set against a brute-force model of the definition in include/g2s.h
(tests/graph_reach_cases.py), k-mer by k-mer; the modes; the argument errors; the cap; g2s_scaffolds_reach against a
model of the scaffold scanner in every state it can be in.  CPU only (G2S_HOST_BUILD=1);
tests/test_gpu_graph_reach.py runs the device search against this path."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import cases  # noqa: E402
import graph_reach_cases as GC  # noqa: E402
import reach_cases as RC  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402

ERR_ARG = -1  # G2S_ERR_ARG (include/g2s.h)
TOO_MANY = "too many k-mers for 32-bit oriented node ids"


@pytest.fixture(autouse=True)
def _host_build(monkeypatch):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    monkeypatch.delenv("G2S_BUILD_MAX_KMERS", raising=False)
    monkeypatch.delenv("G2S_BUILD_REACH", raising=False)


def _outside(k, gaps):
    rng = cases.SplitMix(k)
    return [cases.random_dna(rng, k) for _ in range(20)] + [gaps["D"]["left"][:k]]


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", GC.KS)
def test_the_kept_set_equals_the_model(k, solid):
    seqs, gaps = GC.workload(k, solid)
    for name, records in GC.scenarios(k, gaps).items():
        full, kept = GC.model(seqs, records, k, solid)
        assert 0 < len(kept) < len(full), (name, len(kept), len(full))
        u = P.Graph.from_seqs(seqs, k, solid, reach=GC.reach_of(P, records))
        try:
            info = P.test_last_graph_reach()
            GC.assert_matches_model(P, u, full, kept, _outside(k, gaps))
            assert u.bounded
        finally:
            u.free()
        seeds = sum(len(RC.seeds_of(g, k)) for g, _ in records)
        in_full = sum(1 for g, _ in records for x in RC.seeds_of(g, k) if x in full)
        assert info == dict(records=len(records), seeds=seeds, seeds_in_full=in_full, full_kmers=len(full), kept_kmers=len(kept),
                            levels=info["levels"], passes=0, regrowths=0, on_device=0, ms_search=info["ms_search"]), name
        assert info["levels"] <= max(r for _, r in records)
        if name == "absent_seed":
            assert in_full < seeds
        if name == "twice":   # the larger radius wins: the graph of that record alone
            small = len(GC.model(seqs, records[:1], k, solid)[1])  # (k < 11: 2^k possible k-mers, a ball may hold them all)
            assert kept == GC.model(seqs, records[1:], k, solid)[1] and (len(kept) > small or (k < 11 and len(kept) == small))
        if name == "staggered":  # the balls overlap, and neither holds the other
            a, b = GC.model(seqs, records[:1], k, solid)[1], GC.model(seqs, records[1:], k, solid)[1]
            assert a & b and (k < 11 or (a - b and b - a))
        if name == "late":    # the first record's search has died out when the second enters
            first = GC.model(seqs, records[:1], k, solid)[1]
            assert first == GC.ball(full, RC.seeds_of(records[0][0], k), records[0][1] - records[1][1] - 1)
            assert not first & GC.model(seqs, records[1:], k, solid)[1]


@pytest.mark.parametrize("k", [5, 31, 64])
def test_no_seed_in_the_graph_gives_an_empty_graph(k):
    seqs, gaps = GC.workload(k, 1)
    for reach in ([(gaps["D"], 5)], []):
        u = P.Graph.from_seqs(seqs, k, 1, reach=GC.reach_of(P, reach))
        try:
            info = P.test_last_graph_reach()
            assert u.num_kmers == 0 and u.node(seqs[0][:k]) == P.G2S_INVALID_NODE and u.bounded
            assert info["kept_kmers"] == 0 and info["seeds_in_full"] == 0 and info["records"] == len(reach)
            assert info["full_kmers"] == len(GC.model(seqs, [], k, 1)[0])
        finally:
            u.free()


def test_the_largest_radius_an_int32_holds():
    """entry levels are indexed sparsely: a record at 2^31 - 1 keeps its seeds' whole component, one at 3 enters at the
    end of a search that has long died out, and nothing is sized by the radius"""
    k = 31
    seqs, gaps = GC.workload(k, 1)
    records = [(gaps["A"], 2 ** 31 - 1), (gaps["E"], 3)]
    full, kept = GC.model(seqs, [(gaps["A"], 10 ** 6), (gaps["E"], 3)], k, 1)
    assert 0 < len(kept) < len(full)
    u = P.Graph.from_seqs(seqs, k, 1, reach=GC.reach_of(P, records))
    try:
        GC.assert_matches_model(P, u, full, kept)
    finally:
        u.free()
    recs = P.scaffolds_reach(">a\n" + seqs[0][:200] + "NNNN" + seqs[0][204:400] + "\n", k, 10, 2 ** 31 - 1)
    assert [r for _, r in recs] == [2 ** 31 - 1]


@pytest.mark.parametrize("k,r", [(4, 2), (32, 7), (64, 7)])
def test_a_palindrome_on_the_rim(k, r):
    seqs, gap, pal = GC.palindrome_case(k, r)
    assert RC.canon(pal) == pal == RC._rc(pal)
    for radius in (r - 1, r, r + 1):
        full, kept = GC.model(seqs, [(gap, radius)], k, 1)
        assert (pal in kept) == (radius >= r), "the palindrome is not at distance %d" % r
        assert 0 < len(kept) < len(full)
        u = P.Graph.from_seqs(seqs, k, 1, reach=[(GC.gap_obj(P, gap), radius)])
        try:
            GC.assert_matches_model(P, u, full, kept)
        finally:
            u.free()


@pytest.mark.parametrize("k", [5, 31, 32, 65])
def test_never_and_auto_under_the_cap_are_the_plain_build(k):
    seqs, gaps = GC.workload(k, 2)
    reach = GC.reach_of(P, GC.scenarios(k, gaps)["staggered"])
    plain = P.Graph.from_seqs(seqs, k, 2)
    try:
        for mode in (P.REACH_NEVER, P.REACH_AUTO):
            u = P.Graph.from_seqs(seqs, k, 2, reach=reach, reach_mode=mode)
            try:
                assert not u.bounded
                GC.assert_same_graph(u, plain)
                assert [u.node_string(v) for v in range(2 * u.num_kmers)] == [plain.node_string(v) for v in range(2 * plain.num_kmers)]
            finally:
                u.free()
    finally:
        plain.free()


def test_argument_errors():
    seqs, gaps = GC.workload(31, 1)
    bad = [(GC.gap_obj(P, gaps["A"]), 3), (GC.gap_obj(P, gaps["B"]), -1)]
    for mode in (P.REACH_ALWAYS, P.REACH_NEVER, P.REACH_AUTO):
        with pytest.raises(P.G2SError) as e:
            P.Graph.from_seqs(seqs, 31, 1, reach=bad, reach_mode=mode)
        assert e.value.code == ERR_ARG and "negative radius" in str(e.value)
    with pytest.raises(P.G2SError) as e:
        P.Graph.from_seqs(seqs, 31, 1, reach=bad[:1], reach_mode=7)
    assert e.value.code == ERR_ARG


def test_the_cap_applies_to_the_kept_set(monkeypatch):
    k = 31
    seqs, gaps = GC.workload(k, 1)
    records = GC.scenarios(k, gaps)["staggered"]
    full, kept = GC.model(seqs, records, k, 1)
    reach = GC.reach_of(P, records)
    monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(len(full)))  # (a set is refused from the cap on: the whole one is)
    with pytest.raises(P.G2SError) as e:
        P.Graph.from_seqs(seqs, k, 1)
    assert e.value.code == ERR_ARG and TOO_MANY in str(e.value)
    with pytest.raises(P.G2SError):
        P.Graph.from_seqs(seqs, k, 1, reach=reach, reach_mode=P.REACH_NEVER)
    for mode, env in ((P.REACH_ALWAYS, None), (P.REACH_AUTO, None), (P.REACH_AUTO, "1")):
        if env is not None:
            monkeypatch.setenv("G2S_BUILD_REACH", env)
        u = P.Graph.from_seqs(seqs, k, 1, reach=reach, reach_mode=mode)
        try:
            assert u.bounded
            GC.assert_matches_model(P, u, full, kept)
        finally:
            u.free()
    monkeypatch.setenv("G2S_BUILD_REACH", "0")   # AUTO made NEVER: today's failure
    with pytest.raises(P.G2SError):
        P.Graph.from_seqs(seqs, k, 1, reach=reach, reach_mode=P.REACH_AUTO)
    monkeypatch.delenv("G2S_BUILD_REACH")
    monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(len(kept)))  # the kept set at the cap: the same refusal
    with pytest.raises(P.G2SError) as e:
        P.Graph.from_seqs(seqs, k, 1, reach=reach)
    assert e.value.code == ERR_ARG and TOO_MANY in str(e.value)
    monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(len(kept) + 1))
    P.Graph.from_seqs(seqs, k, 1, reach=reach).free()


# ---- g2s_scaffolds_reach against the scanner (gap2seq_amd/csrc/g2s_execute.cpp, Gap2Seq.cpp:340-423) in every state

def _runs(seq):
    out, i = [], 0
    while i < len(seq):
        if seq[i] in "Nn":
            j = i
            while j < len(seq) and seq[j] in "Nn":
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


def scanner_jobs(seq, k, fuz):
    """per N-run, every (kmer_start, lmf, rmf) the scanner can hand the fill: the previous gap may have been filled with
    any right_fuz in [0, its rmf], or not at all"""
    jobs, states = [], {0}
    for istart, iend in _runs(seq):
        rmf = min(len(seq) - (iend + k), fuz)
        ok = rmf >= 0 and iend + k + rmf <= len(seq) and not any(c in "Nn" for c in seq[iend:iend + k + rmf])
        mine, nxt = set(), {iend}
        for sprev in states:
            lmf = min(istart + k - sprev, fuz)
            start = istart - k - lmf
            if start >= sprev and ok:
                mine.add((start, lmf, rmf))
                nxt |= {iend + rf for rf in range(rmf + 1)}
        jobs.append(mine)
        states = nxt
    return jobs


def scaffold_texts():
    rng = cases.SplitMix(31337)
    d = lambda n: cases.random_dna(rng, n)  # noqa: E731
    k, fuz = 11, 4
    # (a gap is a job only with k + rmf clean bases behind it; the next gap is one only while its flank starts at or behind
    # the previous gap's end + right_fuz: runs k + fuz + 2 apart make that depend on the previous right_fuz)
    texts = {
        "adjacent": (k, fuz, ">a\n" + d(40) + "NNNN" + d(k + fuz + 2) + "NN" + d(k + fuz - 1) + "NNNNN" + d(k + fuz) + "N" + d(3) + "N" + d(50) + "\n"),
        "ends": (k, fuz, ">a\nNNN" + d(k + fuz + 1) + "NN" + d(30) + "NNNN" + d(k + 1) + "NN\n>b\n" + d(k + fuz + 3) + "NNN" + d(k) + "\n"),
        "barrier": (4, 9, ">a\n" + d(30) + "NNN" + d(13) + "NN" + d(17) + "NNNN" + d(14) + "N" + d(40) + "\n"),
        "lower": (k, fuz, ">a\n" + d(30) + "nnNn" + d(k + fuz + 1) + "n" + d(40) + "\n>empty\n\n>c\n" + d(25) + "\n"),
    }
    return texts


@pytest.mark.parametrize("name", sorted(scaffold_texts()))
@pytest.mark.parametrize("d_err", [0, 50])
def test_scaffolds_reach_covers_every_state_of_the_scanner(name, d_err):
    k, fuz, text = scaffold_texts()[name]
    records = P.scaffolds_reach(text, k, fuz, d_err)
    seqs = [ln for ln in text.splitlines() if not ln.startswith(">")]
    at, checked = 0, 0
    for seq in seqs:
        runs = _runs(seq)
        jobs = scanner_jobs(seq, k, fuz)
        prev_end = 0
        for (istart, iend), mine in zip(runs, jobs):
            gap, radius = records[at]
            at += 1
            a = max(prev_end, istart - k - fuz, 0)
            assert gap.left == seq[a:istart] and gap.lmf == istart - a - k and gap.gap_len == iend - istart
            for start, lmf, rmf in mine:
                assert a <= start and lmf <= gap.lmf and rmf == gap.rmf
                assert seq[start:istart] in gap.left and gap.left.endswith(seq[start:istart])
                assert gap.right == seq[iend:iend + k + rmf]
                assert radius >= max(0, gap.gap_len + d_err) + lmf + rmf
                # the fill's seeds are among the record's
                fill = dict(left=seq[start:istart], right=gap.right, gap_len=gap.gap_len, lmf=lmf, rmf=rmf)
                rec = dict(left=gap.left, right=gap.right, gap_len=gap.gap_len, lmf=gap.lmf, rmf=gap.rmf)
                assert set(RC.seeds_of(fill, k)) <= set(RC.seeds_of(rec, k))
                checked += 1
            if not mine:   # nothing the scanner can fill: whatever the record says costs at most k-mers
                assert radius >= 0
            prev_end = iend
    assert at == len(records) and checked > 0
