"""GPU tests of phase D3's SHORT ROUTE (run with `-m gpu` on an MI355X): a list of up to 768 gaps on one session, not a
set list and not in flight, has no g2s_d3_back between its tables' kernel and its trace kernel — every workgroup of
g2s_d3_trace<4, true> walks the offsets' chain up to its own gap itself, hands its gap to the host where that finishes
it, and the workgroup that completes the ticket publishes the hand-over's count (gap2seq_amd/csrc/d3_device.hip).

Every case compares every gap's whole result — count, fuz values, flags, draws, fill text with case, subgraph statistics
and lengths — three ways: the short route, the route with g2s_d3_back forced by G2S_D3_BACK=1 in the same process, and the
CPU oracle.  Which route a list took is read from the test hook g2s_test_d3_chain_launches.  Everything goes through the
C ABI."""
import pytest

import cases
from test_gpu_parity import _check_batch, _gaps, _parse_scaffolds

pytestmark = pytest.mark.gpu


def _key(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.fill_len, tuple(r.substats), r.phaseC_count,
            tuple(r.lengths), r.backtrace_msg)


def _stats(tm):
    return (tm.xA, tm.sA, tm.xB, tm.sB, tm.xD, tm.sD, tm.seg_tier_gaps, tm.segx_tier_gaps, tm.seg_segments, tm.fill_bytes,
            tm.draw_dependent_gaps, tm.d3_table_entries, tm.host_finished_gaps, tm.resident_launches, tm.resident_fallbacks)


def _v3(product, genome, ngaps, lo, hi, haplotypes=3):
    reads = product.G2S.synth_genome(genome, haplotypes, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    return seqs, _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, ngaps, lo, hi, 20240103))


def _three_ways(product, oracle, monkeypatch, seqs, k, gaps, e, skip=False, allp=True, seed=5, short=True):
    """The list on the short route against the oracle (gap by gap, _check_batch), then on the route with g2s_d3_back
    against the short route's results and statistics.  short: whether the list qualifies for the short route.  Returns
    the two timing records."""
    monkeypatch.delenv("G2S_D3_BACK", raising=False)
    got = {}

    def run_short(sess, structs):
        before = product.test_d3_chain_launches()
        res, tm = sess.fill_batch(structs, True)
        got["keys"], got["taken"] = [_key(r) for r in res], product.test_d3_chain_launches() - before
        return res, tm

    _, _, tm_new, _, _ = _check_batch(product, oracle, seqs, k, gaps, e, skip, allp, seed=seed, run_product=run_short)
    assert tm_new.resident_launches == 1 and tm_new.resident_fallbacks == 0
    assert got["taken"] == (1 if short else 0)
    monkeypatch.setenv("G2S_D3_BACK", "1")
    pg = product.Graph.from_seqs(seqs, k, 1)
    sess = product.Session(pg, 0, d_err=e, skip_confident=skip, all_paths=allp, randseed=seed)
    try:
        before = product.test_d3_chain_launches()
        res, tm_old = sess.fill_batch(_gaps(product, gaps), True)
        assert product.test_d3_chain_launches() == before
    finally:
        sess.destroy()
        pg.free()
    assert [_key(r) for r in res] == got["keys"]
    assert _stats(tm_old) == _stats(tm_new)
    return tm_new, tm_old


@pytest.mark.parametrize("n", [256, 257, 768, 769])
def test_list_lengths_at_the_routes_bounds(product, oracle, monkeypatch, n):
    """256 gaps (the shortest list that is finished on the device by default), 257, 768 (the longest on the short route:
    the trace kernel's four-wave instantiation) and 769, which keeps g2s_d3_back."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    seqs, gaps = _v3(product, 300000, 769, 60, 300)
    tm, _ = _three_ways(product, oracle, monkeypatch, seqs, 31, gaps[:n], 300, short=n <= 768)
    assert tm.draw_dependent_gaps > 0


def test_a_list_without_a_draw_dependent_gap(product, oracle, monkeypatch):
    """One haplotype, no bubbles: no gap's draw count depends on the draws — V = 0, T = 0, a chain of no steps."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    seqs, gaps = _v3(product, 200000, 300, 100, 600, haplotypes=1)
    tm, _ = _three_ways(product, oracle, monkeypatch, seqs, 31, gaps, 500)
    assert tm.draw_dependent_gaps == 0 and tm.d3_table_entries == 0


def test_the_chain_through_device_memory(product, oracle, monkeypatch):
    """G2S_TEST_CHAIN_ROOM=0: no room for the tables in the trace kernel's LDS — every workgroup walks them where they
    lie, with the same result."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.setenv("G2S_TEST_CHAIN_ROOM", "0")
    seqs, gaps = _v3(product, 200000, 500, 100, 900)
    tm, _ = _three_ways(product, oracle, monkeypatch, seqs, 31, gaps, 500)
    assert tm.draw_dependent_gaps > 0 and tm.d3_table_entries >= tm.draw_dependent_gaps


def test_a_skip_rule_and_a_bad_flank_in_the_lists_middle(product, monkeypatch):
    """Every second gap carries a skip rule (not attempted when the gap in front of it was filled with a right fuz above
    0, Gap2Seq.cpp:369 — every fourth gap is: the scan takes a skipped gap's draws out of every offset behind it), and the gap in the list's
    middle has a left flank of five bases (a bad flank: never launched).  The short route, the route with g2s_d3_back and
    the host path of the same library (the oracle's fill_gap knows no skip rule; the parity suite pins the host path)."""
    seqs, gaps = _v3(product, 200000, 400, 100, 900)
    flip = str.maketrans("ACGT", "CATG")
    structs = []
    for i, g in enumerate(gaps):
        # (every fourth gap's right flank begins with three bases that are not the genome's: it is reached at a fuz of 3
        # or more, which is above the gap behind it's threshold)
        right = g["right"][:3].translate(flip) + g["right"][3:] if i % 4 == 0 else g["right"]
        structs.append(product.Gap(g["left"], right, g["gap_len"], g["lmf"], g["rmf"], 0 if i % 2 else -1))
    structs[200] = product.Gap(gaps[200]["left"][-5:], gaps[200]["right"], gaps[200]["gap_len"], 10, 10, -1)
    pg = product.Graph.from_seqs(seqs, 31, 1)
    out, taken = {}, {}
    try:
        for how in ("short", "back", "host"):
            monkeypatch.setenv("G2S_RESIDENT", "0" if how == "host" else "1")
            monkeypatch.setenv("G2S_D3_BACK", "1" if how == "back" else "0")
            sess = product.Session(pg, 0, d_err=500, randseed=3)
            before = product.test_d3_chain_launches()
            res, tm = sess.fill_batch(structs, True)
            out[how], taken[how] = [_key(r) for r in res], product.test_d3_chain_launches() - before
            assert tm.resident_launches == (0 if how == "host" else 1) and tm.resident_fallbacks == 0
            if how == "short":
                assert res[200].flags & product.G2S_GAP_BAD_FLANK
                assert sum(1 for r in res if r.flags & product.G2S_GAP_SKIPPED) > 0
                assert sum(1 for r in res[201:] if r.draws > 1) > 0 and tm.draw_dependent_gaps > 0
            sess.destroy()
    finally:
        pg.free()
    assert taken == {"short": 1, "back": 0, "host": 0}
    assert out["short"] == out["host"] and out["back"] == out["host"]


@pytest.mark.parametrize("mode", ["best_only", "unique"])
def test_best_only_and_unique_paths_lists(product, oracle, monkeypatch, mode):
    """-best-only against the oracle; -unique (which the oracle's fill_gap does not take) against the host path of the
    same library, which the parity suite pins to the reference."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    seqs, gaps = _v3(product, 200000, 600, 100, 900)
    if mode == "best_only":
        tm, _ = _three_ways(product, oracle, monkeypatch, seqs, 31, gaps, 500, allp=False)
        assert tm.draw_dependent_gaps > 0
        return
    out, taken = {}, {}
    pg = product.Graph.from_seqs(seqs, 31, 1)
    try:
        for how in ("short", "back", "host"):
            monkeypatch.setenv("G2S_RESIDENT", "0" if how == "host" else "1")
            monkeypatch.setenv("G2S_D3_BACK", "1" if how == "back" else "0")
            sess = product.Session(pg, 0, d_err=500, randseed=3, unique_paths=True)
            before = product.test_d3_chain_launches()
            res, tm = sess.fill_batch(_gaps(product, gaps), True)
            out[how], taken[how] = [_key(r) for r in res], product.test_d3_chain_launches() - before
            assert tm.resident_launches == (0 if how == "host" else 1) and tm.resident_fallbacks == 0
            sess.destroy()
    finally:
        pg.free()
    assert taken == {"short": 1, "back": 0, "host": 0}
    assert out["short"] == out["host"] and out["back"] == out["host"]


@pytest.mark.parametrize("d2", [None, "1"])
def test_toy_graphs_with_closures_for_the_host(product, oracle, monkeypatch, d2):
    """Small k, tandem and inverted repeats: closures that hold a k-mer at two depths.  By default a short list's are the
    host threads' — handed over by the gap's own workgroup of the trace kernel, the count published by the ticket —; with
    G2S_DEVICE_D2=1 g2s_d2_* analyses them beside phase D3's first kernels and the workgroups wait for its verdicts."""
    monkeypatch.setenv("G2S_RESIDENT", "1")
    if d2 is None:
        monkeypatch.delenv("G2S_DEVICE_D2", raising=False)
    else:
        monkeypatch.setenv("G2S_DEVICE_D2", d2)
    handed = 0
    for seed in (1, 4, 7):
        k = [9, 11, 13, 15, 17, 21][seed % 6]
        seqs = cases.toy_genome(seed, 1500, k, repeats=seed % 3, tandem=seed % 2, inverted=int(seed % 4 == 0), snp_every=(0 if seed % 2 else 97))
        e = [0, 9, 20, 31][seed % 4] + k
        gaps = cases.cut_gaps(seed, seqs[0], k, fuz=seed % 5 + 1, ngaps=60, min_len=1, max_len=80, d_err=e)
        tm, _ = _three_ways(product, oracle, monkeypatch, seqs, k, gaps, e)
        handed += tm.host_finished_gaps
    assert (handed > 0) == (d2 is None)


def test_one_deep_gap_reruns_in_the_large_variant(product, oracle, monkeypatch):
    """A 600-gap list with one gap in its middle that outgrows the regular tier (6 kbp: more than 512 segments) and runs
    again in the large variant behind the fill kernel: it rejoins the list's phase D3 on the short route."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    reads = product.G2S.synth_genome(1000000, 3, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    gaps = _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, 600, 200, 1000, 20240103))
    deep = _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, 3, 6000, 6000, 77))
    gaps = gaps[:300] + deep[:1] + gaps[300:599]
    tm, _ = _three_ways(product, oracle, monkeypatch, seqs, 31, gaps, 500, seed=1)
    assert tm.segx_tier_gaps >= 1 and tm.seg_tier_gaps + tm.segx_tier_gaps == 600 and tm.watchdog_gaps == 0


def test_three_lists_on_one_session(product, monkeypatch):
    """500, 300 and 500 gaps in a row on one session: what the longer list left in the work areas — class words, offsets,
    tables, the ticket — must not reach the shorter one, nor the third list the first's.  Against the same three calls with
    g2s_d3_back, and against the host path."""
    seqs, gaps = _v3(product, 200000, 500, 100, 900)
    structs = _gaps(product, gaps)
    lists = (structs, structs[100:400], structs)
    pg = product.Graph.from_seqs(seqs, 31, 1)
    out, taken = {}, {}
    try:
        for how in ("short", "back", "host"):
            monkeypatch.setenv("G2S_RESIDENT", "0" if how == "host" else "1")
            monkeypatch.setenv("G2S_D3_BACK", "1" if how == "back" else "0")
            sess = product.Session(pg, 0, d_err=500, randseed=3)
            before = product.test_d3_chain_launches()
            out[how] = [[_key(r) for r in sess.fill_batch(l, pinned=True)] for l in lists]
            taken[how] = product.test_d3_chain_launches() - before
            sess.destroy()
    finally:
        pg.free()
    assert taken == {"short": 3, "back": 0, "host": 0}
    assert out["short"] == out["host"] and out["back"] == out["host"]


def test_the_768_gap_list_thirty_times():
    """The 768-gap list thirty times through one session of the product build and of the two race-hunting builds (waves
    delayed at random; every barrier a full one): every call's results equal the first call's, and the first call's are
    the same in all three builds.  (A child process per build: a process holds one build of the library.)"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import hashlib, json, sys
sys.path[:0] = [%r, %r]
from gap2seq_amd import lib as P
from test_gpu_parity import _gaps, _parse_scaffolds
reads = P.G2S.synth_genome(300000, 3, 20240101)
seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
gaps = _gaps(P, _parse_scaffolds(P.G2S.synth_gaps(reads, 31, 10, 768, 60, 300, 20240103)))
pg = P.Graph.from_seqs(seqs, 31, 1)
sess = P.Session(pg, 0, d_err=300, randseed=5)
before = P.test_d3_chain_launches()
digests = []
for it in range(30):
    sess.srand(5)
    res = sess.fill_batch(gaps)
    now = repr([(r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, tuple(r.substats), r.phaseC_count, tuple(r.lengths)) for r in res])
    digests.append(hashlib.sha256(now.encode()).hexdigest())
print(json.dumps(dict(digests=digests, taken=P.test_d3_chain_launches() - before, filled=sum(1 for r in res if r.count > 0))))
""" % (root, os.path.join(root, "tests"))
    firsts = {}
    for sub in ("", "_jit", "_par"):
        path = os.path.join(root, "gap2seq_amd", sub, "libg2s_hip.so")
        if not os.path.exists(path):
            pytest.fail("%s is missing: __graft_entry__.build() makes it" % path)
        env = dict(os.environ, G2S_LIBRARY=path)
        for v in ("G2S_D3_BACK", "G2S_RESIDENT", "G2S_TEST_CHAIN_ROOM", "G2S_DEVICE_D2", "G2S_TRACE_WAVES"):
            env.pop(v, None)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, "%s: %s" % (sub or "product", p.stderr[-2000:])
        got = json.loads(p.stdout.strip().splitlines()[-1])
        assert got["taken"] == 30 and got["filled"] > 500, (sub, got["taken"], got["filled"])
        differ = [i for i, d in enumerate(got["digests"]) if d != got["digests"][0]]
        assert not differ, "%s: calls %r differ from the first" % (sub or "product", differ)
        firsts[sub] = got["digests"][0]
    assert len(set(firsts.values())) == 1, "the builds disagree: %r" % firsts
