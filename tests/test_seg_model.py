"""The algorithm of the segment tier (tests/seg_model.py) against the CPU oracle, without a GPU:
DP table, work counters, phase C outcome, Q7 and — through the host half of phase D
(g2s_test_post_closure) — fill, fuz values, draw counts, safe/unsafe case and subgraph statistics."""
import pytest

import cases
import seg_model as M


def _model_gap(pg, k, g, e, allp=True, skip=False):
    lmf, rmf = g["lmf"], g["rmf"]
    left, right = g["left"], g["right"]
    lseeds = [pg.node(left[d:d + k]) for d in range(lmf + 1)]
    rseeds = [pg.node(right[len(right) - k - d:len(right) - d]) for d in range(rmf + 1)]
    targets = [pg.node(right[d:d + k]) for d in range(rmf + 1)]
    return M.Gap(g["gap_len"], e, lmf, rmf, lseeds, rseeds, targets, all_paths=allp, skip_confident=skip)


STATS = {}


def _parent_sets(records, xp):
    extra = {}
    for x in xp:
        extra.setdefault(x >> 32, set()).add(x & 0xFFFFFFFF)
    out = []
    for i, (_, _, _, pred) in enumerate(records):
        out.append(set() if pred < 0 else ({pred & M.SUB_MORE - 1} | extra.get(i, set())))
    return out


def check_config(product, oracle, seqs, k, gaps, e, allp=True, skip=False, seed=5, stats=None):
    pg = product.Graph.from_seqs(seqs, k, 1)
    og = oracle.OracleGraph(seqs, k, 1)
    tb = M.Tables(product, pg)
    params = product.make_params(d_err=e, skip_confident=skip, all_paths=allp, randseed=seed)
    compared = nq7 = 0
    nseg_path = STATS.setdefault("on_segments", [0])
    try:
        for gi, g in enumerate(gaps):
            rng = oracle.OracleRng(seed)
            o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], e, g["lmf"], g["rmf"], skip, allp, dump=True)
            rng.free()
            mg = _model_gap(pg, k, g, e, allp, skip)
            m = M.fill_model(tb, mg, stats=stats)
            if o.info.q7:
                nq7 += 1
                continue
            what = "gap %d" % gi
            want = sorted((s, d, c) for s, d, c in o.states)
            got = sorted((pg.node_string(v), d, c) for v, d, c in M.expand_states(m))
            assert got == want, what
            assert (m.xB, m.sB) == (o.info.ctr[2], o.info.ctr[3]), what
            assert not m.q7, what + ": the model flags Q7, the oracle does not"
            assert m.c_count == o.info.phaseC_count and m.lengths == o.lengths, what
            if o.phase_d:
                assert m.reached_j == o.info.reached_fuz and m.final_d == o.info.final_d, what
                pgap = product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])
                # the host's expansion of the closure segments = the model's per-state records (the side
                # list as a set per state: the kernel lists a state's parents in arrival order)
                recs, xps = product.test_seg_expand(pg, params, pgap, m.compact, m.lengths, m.reached_j, len(m.records),
                                                    len(m.xp))
                assert [x[:3] for x in recs] == [x[:3] for x in m.records], what
                assert _parent_sets(recs, xps) == _parent_sets(m.records, sorted(m.xp)), what
                r = product.test_post_closure(pg, params, pgap, recs, xps, m.c_count, m.lengths, m.reached_j, m.final_d,
                                              seed, 0)
                # and the analysis + traceback run on the segments themselves (what the batch path does
                # whenever no k-mer occurs at two depths of the closure)
                r2, on_segments = product.test_post_segments(pg, params, pgap, m.compact, m.c_count, m.lengths, m.reached_j,
                                                             m.final_d, seed, 0)
                if on_segments:
                    nseg_path[0] += 1
                    assert (r2.count, r2.left_fuz, r2.right_fuz, r2.draws, r2.fill, r2.flags) == \
                        (r.count, r.left_fuz, r.right_fuz, r.draws, r.fill, r.flags), what
                    if not skip:
                        assert r2.substats == r.substats, what
                assert r.count == o.count, what
                assert (r.left_fuz, r.right_fuz, r.draws) == (o.left_fuz, o.right_fuz, o.info.draws), what
                assert r.fill == o.fill, what
                if not skip:
                    assert r.substats == o.substats, what
            compared += 1
    finally:
        pg.free()
        og.free()
    return compared, nq7


@pytest.mark.parametrize("seed", range(12))
def test_model_toy_graphs_all_modes(product, oracle, seed):
    k = [5, 7, 9, 11, 13, 15][seed % 6]
    seqs = cases.toy_genome(seed, 900, k, repeats=seed % 4, tandem=seed % 3, inverted=int(seed % 5 == 0),
                            snp_every=(0 if seed % 2 else 83))
    e = [0, 4, 9, 20, 31][seed % 5] + k
    # (the Python model is slow on the tangled graphs of k <= 9: fewer gaps there)
    gaps = cases.cut_gaps(seed, seqs[0], k, fuz=seed % 5 + 1, ngaps=40 if k >= 11 else 10, min_len=1, max_len=60, d_err=e)
    total = 0
    for skip, allp in ((False, True), (False, False), (True, True)):
        c, q = check_config(product, oracle, seqs, k, gaps, e, allp, skip)
        assert c + q == len(gaps)
        total += c
    assert total >= (90 if k >= 11 else 0)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_model_k31_default_parameters(product, oracle, variant):
    reads = product.G2S.synth_genome(200000, variant, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    from test_gpu_parity import _parse_scaffolds
    gaps = _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, 40, 50, 400, 20240103))
    stats = []
    before = STATS.setdefault("on_segments", [0])[0]
    c, q = check_config(product, oracle, seqs, 31, gaps, 500, stats=stats)
    assert c == 40
    assert STATS["on_segments"][0] - before >= 36  # nearly every closure has each k-mer at one depth only


def test_model_repeated_kmers_are_analysed_on_runs(product, oracle):
    """Closures in which a k-mer occurs at several depths (tandem repeats, bubbles of unequal length): the
    host analyses them on runs of k-mers (post.cpp: seg_analyze_runs).  check_config compares fill, flags,
    draws and the subgraph statistics of that analysis with the per-state one for every closure; here nearly
    every gap's closure stays on segments (with the run analysis switched off, G2S_STATE_D2=1, a third of
    this set falls back to per-state records)."""
    k = 11
    seqs = cases.toy_genome(21, 3000, k, repeats=4, tandem=6, snp_every=97)
    gaps = cases.cut_gaps(10, seqs[0], k, fuz=7, ngaps=40, min_len=1, max_len=80, d_err=30)
    before = STATS.setdefault("on_segments", [0])[0]
    c, q = check_config(product, oracle, seqs, k, gaps, 30)
    assert c + q == 40
    assert STATS["on_segments"][0] - before >= 25


def test_model_tandem_flanks_and_fuz_extremes(product, oracle):
    """Q6 territory (seed states reached by the DP as well) and fuz 0 / large fuz."""
    k = 11
    seqs = cases.toy_genome(21, 3000, k, repeats=4, tandem=6, snp_every=97)
    for fuz in (0, 1, 7, 15):
        gaps = cases.cut_gaps(3 + fuz, seqs[0], k, fuz=fuz, ngaps=40, min_len=1, max_len=80, d_err=30)
        c, q = check_config(product, oracle, seqs, k, gaps, 30)
        assert c + q == 40 and c >= 20


@pytest.mark.parametrize("k,length", [(5, 60), (5, 100), (7, 200)])
def test_model_small_k_without_strand_collisions(product, oracle, k, length):
    """k = 5 and 7 on genomes over {A, C}: no gap is a Q7 case, so every one is compared — dense graphs,
    closures full of cycles, saturating counts (the toy graphs above leave almost nothing to compare at these k)."""
    for seed in range(3):
        seqs = [cases.one_strand_genome(seed, length)]
        e = [0, 4, 9, 20, 31][seed % 5] + k
        gaps = cases.cut_gaps(seed, seqs[0], k, fuz=seed % 3 + 1, ngaps=16, min_len=1, max_len=length // 4, d_err=e)
        for skip, allp in ((False, True), (False, False), (True, True)):
            c, q = check_config(product, oracle, seqs, k, gaps, e, allp, skip)
            assert (c, q) == (len(gaps), 0)


def _ladder_model(product, oracle, lad, e, allp=True, skip=False):
    g = lad["gap"]
    pg = product.Graph.from_seqs(lad["seqs"], 31, 1)
    og = oracle.OracleGraph(lad["seqs"], 31, 1)
    try:
        tb = M.Tables(product, pg)
        mg = _model_gap(pg, 31, g, e, allp, skip)
        rs = M.right_set(tb, mg)
        label = M.right_entries(tb, mg)
        assert M.entries_to_set(tb, mg, label) == rs
        m = M.fill_model(tb, mg, rs)
        rng = oracle.OracleRng(5)
        o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], e, g["lmf"], g["rmf"], skip, allp)
        rng.free()
    finally:
        pg.free()
        og.free()
    return m, len(label), o


@pytest.mark.parametrize("name", sorted(cases.EDGE_LADDERS))
def test_edge_ladders_sit_where_the_gpu_tests_say(product, oracle, name):
    """Every planted gap of cases.EDGE_LADDERS (tests/test_gpu_edges.py) at its capacity: the segments the left DP
    logs, the right set's entries, the closure's segments and phase C's count are the model's, and the model's
    count is the oracle's (2^29 exactly; 2^30 and 2^31 saturate at MAX_PATHS)."""
    lad, want = cases.edge_ladder(name)
    m, n_entries, o = _ladder_model(product, oracle, lad, 10)
    assert not m.q7 and not o.info.q7
    assert (m.n_seg, n_entries, len(m.compact)) == (want["nseg"], want["nA"], want["ncl"])
    assert m.c_count == o.info.phaseC_count == want.get("count", cases.MAX_PATHS)
    assert m.lengths == o.lengths and o.count > 0
    if lad["paths"] is not None:
        assert o.count == min(lad["paths"], cases.MAX_PATHS)


def test_edge_ladders_step_by_one_across_each_capacity():
    """The table holds cap - 1, cap and cap + 1 for every capacity the model sees."""
    got = {}
    for name, (_, want) in cases.EDGE_LADDERS.items():
        for key in ("nseg", "nA", "ncl"):
            got.setdefault(key, set()).add(want[key])
    for cap in (64, 128, 192, 512):
        assert {cap - 1, cap, cap + 1} <= got["nseg"], cap
    assert {255, 256, 257} <= got["nA"]
    assert {255, 256, 257} <= got["ncl"]
    counts = {w.get("count", cases.MAX_PATHS) for _, w in cases.EDGE_LADDERS.values()}
    assert 1 << 29 in counts and cases.MAX_PATHS == (1 << 30) - 2


@pytest.mark.parametrize("name", ["paths2^29", "paths2^30", "paths2^31", "seg193", "indel20"])
def test_edge_ladders_in_every_mode(product, oracle, name):
    """The count ladders and two closures the host analyses, with -best-only and with the skip rule: the model
    (the host half of phase D included) equals the oracle in every field."""
    lad, want = cases.edge_ladder(name)
    for skip, allp in ((False, True), (False, False), (True, True)):
        c, q = check_config(product, oracle, lad["seqs"], 31, [lad["gap"]], 10, allp, skip)
        assert (c, q) == (1, 0)


def test_edge_ladders_share_one_graph():
    """tests/test_gpu_edges.py runs the planted gaps as one list on one graph, among ordinary gaps: no ladder's
    k-mer is another's or the plain genome's."""
    seqs, gaps, idx = cases.edge_ladder_list(sorted(cases.EDGE_LADDERS), pad=300)
    assert cases.clean_haplotypes(seqs, 31) and len(gaps) == 300 + len(cases.EDGE_LADDERS)
    assert [gaps[i] for i in idx] == cases.edge_ladder_list(sorted(cases.EDGE_LADDERS))[1]


def _limit_facts(product, oracle, name, monkeypatch):
    """Model, right-set entries, merged intervals and oracle result of one row of cases.LIMIT_EDGES."""
    lad, want = cases.limit_edge(name)
    if "M" in want:  # M depends on how the unitigs are numbered: the host build's numbering, on every machine
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
    g = lad["gap"]
    pg = product.Graph.from_seqs(lad["seqs"], 31, 1)
    og = oracle.OracleGraph(lad["seqs"], 31, 1)
    try:
        tb = M.Tables(product, pg)
        mg = _model_gap(pg, 31, g, 10)
        label = M.right_entries(tb, mg)
        rs = M.entries_to_set(tb, mg, label)
        if len(label) < 1000:
            assert rs == M.right_set(tb, mg)
        ivs = M.merged_intervals(tb, mg, label)
        assert {x for lo, hi in ivs for x in range(lo, hi + 1)} == rs
        assert all(b[0] > a[1] + 1 for a, b in zip(ivs, ivs[1:]))  # a hole between any two
        m = M.fill_model(tb, mg, rs)
        rng = oracle.OracleRng(5)
        o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], 10, g["lmf"], g["rmf"], False, True)
        rng.free()
    finally:
        pg.free()
        og.free()
    return m, label, ivs, o, want


@pytest.mark.parametrize("name", sorted(cases.LIMIT_EDGES))
def test_limit_edges_sit_where_the_gpu_tests_say(product, oracle, monkeypatch, name):
    """Every planted gap of cases.FRONTIER_EDGES and cases.SEGW_EDGES (tests/test_gpu_segw_edges.py) at its limit:
    logged segments, right-set entries, closure segments, count, the peak of pending events by each kernel's own
    rule, rounds, and where the table names them merges, sweeps and M are the model's; the model's count and lengths
    are the oracle's and neither sees Q7."""
    m, label, ivs, o, want = _limit_facts(product, oracle, name, monkeypatch)
    assert not m.q7 and not o.info.q7
    got = dict(nseg=m.n_seg, nA=len(label), ncl=len(m.compact), count=m.c_count, ev=m.max_pending, ring=m.ring_peak,
               gen=m.n_gen, merges=m.merges_at_peak, sweeps=m.sweeps, M=len(ivs), straddle=m.rs_round == m.reg_round)
    want = dict(want)
    want.setdefault("count", cases.MAX_PATHS)
    assert {key: got[key] for key in want} == want
    assert m.c_count == o.info.phaseC_count and m.lengths == o.lengths and o.count > 0
    # the regular tier's first limit in phase B, as tests/test_gpu_segw_edges.py expects it from these numbers
    assert m.reg_first == ("log" if want["nseg"] > 16000 else "frontier" if want["ev"] > 64 else None)
    if want.get("sweeps"):
        assert m.sweep_live >= 1  # the table was rebuilt with events pending in it
    if "M" in want:
        # a case tests a level only if its searches reach the ends of the top block: with c = the samples of the top
        # block at or below the key, c = 0 (the first block below), c = the block's last real sample (8 at M = 8^j,
        # 1 at M = 8^j + 1: the last block) and, where there is one, a c in between; answers inside and outside
        firsts = [lo for lo, hi in ivs]
        tops, answers = set(), set()
        for q, inside in m.queries:
            rank, blocks, top = M.rank_blocks(firsts, q)
            assert inside == (rank > 0 and q <= ivs[rank - 1][1])
            assert len(blocks) == 1 + sum(want["M"] > cap for cap in (8, 64, 512, 4096))
            tops.add(top)
            answers.add(inside)
        last = 8 if want["M"] in (8, 64, 512, 4096) else 1
        assert {0, last} <= tops and max(tops) == last and (last == 1 or tops - {0, last}), sorted(tops)
        assert answers == {True, False}


def test_limit_edges_step_by_one_across_each_limit():
    """The tables hold limit - 1, limit and limit + 1 for the lanes of the regular tier and for every capacity of
    the large variant that a Q7-free gap can reach (DESIGN section 6 for the two that none can), and the eight values
    of M around the four level boundaries of the search."""
    col = lambda table, key: {w[key] for _, _, w in table.values() if key in w}
    assert {63, 64, 65} <= col(cases.FRONTIER_EDGES, "ev")
    assert {1024, 1025} <= col(cases.FRONTIER_EDGES, "ring") and max(col(cases.LIMIT_EDGES, "ring")) == 1025
    assert {16383, 16384, 16385} <= col(cases.SEGW_EDGES, "nseg")
    assert {6143, 6144, 6145} <= col(cases.SEGW_EDGES, "nA")
    assert col(cases.SEGW_EDGES, "M") == {8, 9, 64, 65, 512, 513, 4096, 4097}
    rows = cases.FRONTIER_EDGES
    assert rows["ev64merge"][2]["merges"] >= 1 and rows["ev64straddle"][2]["straddle"]
    assert any(w.get("sweeps", 0) >= 1 and w["ring"] == 1024 for _, _, w in rows.values())
    # every over-by-one row is over ONE limit of its kernel, so that its reason bit is that limit's
    for name, (_, _, w) in cases.LIMIT_EDGES.items():
        over = [w["nA"] > 6144, w["nseg"] > 16384, w["ring"] > 1024]
        assert sum(over) <= 1, name


@pytest.mark.parametrize("name", ["ev64merge", "ev64straddle", "ev65", "iv9", "iv65"])
def test_limit_edges_in_every_mode(product, oracle, monkeypatch, name):
    """Small rows with -best-only and with the skip rule, the host half of phase D included: the model equals the
    oracle in every field (DP table, counters, fill, fuz, draws, subgraph statistics)."""
    lad, want = cases.limit_edge(name)
    for skip, allp in ((False, True), (False, False), (True, True)):
        c, q = check_config(product, oracle, lad["seqs"], 31, [lad["gap"]], 10, allp, skip)
        assert (c, q) == (1, 0)


def test_limit_edges_share_one_graph():
    """tests/test_gpu_segw_edges.py runs the frontier rows as one list on one graph among ordinary gaps, and puts
    them with the search-level rows into a long resident list: no row's k-mer is another's or the plain genome's."""
    names = sorted(cases.FRONTIER_EDGES) + sorted(n for n in cases.SEGW_EDGES if n.startswith("iv"))
    seqs, gaps, idx = cases.limit_edge_list(names, pad=300)
    assert cases.clean_haplotypes(seqs, 31) and len(gaps) == 300 + len(names)
    assert [gaps[i] for i in idx] == cases.limit_edge_list(names)[1]
