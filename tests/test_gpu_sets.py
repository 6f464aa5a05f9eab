"""g2s_fill_sets on the GPU: every gap of a list filled in its own read set of a set graph, as a fresh
Gap2Seq-core -reads S(i) -left L -right R -length G -randseed seed would fill it (Gap2Seq.py:133-218 runs one per gap).
Checked gap by gap against the CPU oracle on a graph of S(i) alone (the filled sequence, byte for byte) and against the
product's own single-graph path on a fresh session (every result field); the rand() stream restarts for every gap, so
a gap's result depends neither on its position in the list nor on its neighbours; the switches that pick other kernel
paths change nothing."""
import pytest

import cases
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 7
D_ERR = 100
FUZ = 10


def _workload(k, seed, ngaps, solid=1):
    """(sets, gaps, gap_set): per gap, reads of both haplotypes around the gap plus a window from elsewhere (sets
    overlap); every fourth gap shares the set of the gap in front of it; one gap names an empty set; one set is
    named by no gap."""
    hap = cases.toy_genome(seed, 12000, k, repeats=6, tandem=2, snp_every=350)
    genome = hap[0]
    rng = cases.SplitMix(seed * 31 + k)
    raw = cases.cut_gaps(seed, genome, k, FUZ, ngaps, 10, 160, D_ERR)
    sets, gaps, gap_set = [], [], []
    for i, g in enumerate(raw):
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 150), min(len(genome), pos + g["true_len"] + 150)
        o = rng.randint(0, len(genome) - 400)
        reads = [h[lo:hi] for h in hap] + [genome[o:o + 400]]
        reads = reads * solid
        if i % 4 == 3:
            sets[-1].extend(reads)
        else:
            sets.append(reads)
        gaps.append(g)
        gap_set.append(len(sets) - 1)
    sets.append([genome[:600]] * solid)  # named by no gap
    sets.append([])
    gaps.append(dict(raw[0]))
    gap_set.append(len(sets) - 1)  # the empty set
    return sets, gaps, gap_set


def _gap(product, g):
    return product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])


def _sequence(g, r, unique):
    if r.count > 0 and (not unique or r.count == 1):
        return g["left"][:len(g["left"]) - r.left_fuz] + r.fill
    return g["left"] + "N" * g["gap_len"] + g["right"]


_oracle_cache = {}


def _oracle_sequence(seqs, g, k, solid, opts):
    key = (tuple(seqs), g["left"], g["right"], g["gap_len"], k, solid, tuple(sorted(opts.items())))
    if key not in _oracle_cache:
        if not seqs:
            _oracle_cache[key] = g["left"] + "N" * g["gap_len"] + g["right"]
        else:
            og = O.OracleGraph(seqs, k, solid)
            try:
                fa, _ = O.execute_single(og, g["left"], g["right"], g["gap_len"], k, solid=solid, d_err=D_ERR,
                                         max_fuz=max(g["lmf"], g["rmf"], FUZ), randseed=SEED, **opts)
            finally:
                og.free()
            _oracle_cache[key] = "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))
    return _oracle_cache[key]


def _fields(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.substats, r.phaseC_count, r.lengths)


def _run(product, sets, gaps, gap_set, k, solid, order=None, **opts):
    u = product.Graph.from_sets(sets, k, solid)
    sess = product.Session(u, 0, d_err=D_ERR, randseed=SEED, **opts)
    try:
        order = list(range(len(gaps))) if order is None else order
        res = sess.fill_sets([_gap(product, gaps[i]) for i in order], [gap_set[i] for i in order])
        return {i: r for i, r in zip(order, res)}
    finally:
        sess.destroy()
        u.free()


def _single(product, seqs, g, k, solid, **opts):
    """the product's single-graph path on a fresh session of a graph of S(i) alone"""
    gr = product.Graph.from_seqs(seqs, k, solid)
    sess = product.Session(gr, 0, d_err=D_ERR, randseed=SEED, **opts)
    try:
        return sess.fill_batch([_gap(product, g)])[0]
    finally:
        sess.destroy()
        gr.free()


_OPT = {"plain": {}, "all_upper": dict(skip_confident=True), "best_only": dict(all_paths=False),
        "unique": dict(unique_paths=True)}
_ORC = {"plain": {}, "all_upper": dict(skip_confident=True), "best_only": dict(all_paths=False),
        "unique": dict(unique_paths=True)}


def _check(product, sets, gaps, gap_set, res, k, solid, opt="plain", n_single=12):
    unique = opt == "unique"
    filled = 0
    for i, g in enumerate(gaps):
        r = res[i]
        want = _oracle_sequence(sets[gap_set[i]], g, k, solid, _ORC[opt])
        assert _sequence(g, r, unique) == want, "gap %d (set %d)" % (i, gap_set[i])
        filled += r.count > 0
        if not sets[gap_set[i]]:
            assert r.count == 0 and r.draws == 0
    assert filled > len(gaps) // 3
    step = max(1, len(gaps) // n_single)
    for i in list(range(0, len(gaps) - 1, step)):
        if sets[gap_set[i]]:
            assert _fields(res[i]) == _fields(_single(product, sets[gap_set[i]], gaps[i], k, solid, **_OPT[opt])), "gap %d" % i


@pytest.mark.parametrize("k,n", [(31, 1), (31, 255), (31, 256), (63, 256), (95, 255)])
def test_fill_sets_against_oracle_gap_by_gap(product, k, n):
    sets, gaps, gap_set = _workload(k, 11 + k, max(1, n - 1))  # (n - 1 gaps + the one that names the empty set)
    assert n == 1 or len(gaps) == n
    if n == 1:  # a list of one gap: the gap and its own set
        sets, gaps, gap_set = [sets[0]], gaps[:1], [0]
    res = _run(product, sets, gaps, gap_set, k, 1)
    if n == 1:
        r = res[0]
        assert _sequence(gaps[0], r, False) == _oracle_sequence(sets[0], gaps[0], k, 1, {})
        assert _fields(r) == _fields(_single(product, sets[0], gaps[0], k, 1))
        return
    _check(product, sets, gaps, gap_set, res, k, 1)


def test_fill_sets_long_list(product):
    """3 072 gaps: a distinct pool of 384 (gap, set) pairs, each named eight times in a shuffled order"""
    k = 31
    sets, gaps, gap_set = _workload(k, 5, 383)
    rng = cases.SplitMix(99)
    order = [i for i in range(len(gaps)) for _ in range(8)]
    for i in range(len(order) - 1, 0, -1):
        j = rng.randint(0, i)
        order[i], order[j] = order[j], order[i]
    assert len(order) == 3072
    u = product.Graph.from_sets(sets, k, 1)
    sess = product.Session(u, 0, d_err=D_ERR, randseed=SEED)
    try:
        res = sess.fill_sets([_gap(product, gaps[i]) for i in order], [gap_set[i] for i in order])
    finally:
        sess.destroy()
        u.free()
    first = {}
    for pos, i in enumerate(order):
        if i in first:
            assert _fields(res[pos]) == _fields(first[i]), "gap %d at %d" % (i, pos)
        else:
            first[i] = res[pos]
    _check(product, sets, gaps, gap_set, first, k, 1, n_single=4)


@pytest.mark.parametrize("opt", ["all_upper", "best_only", "unique"])
def test_fill_sets_options(product, opt):
    k = 31
    sets, gaps, gap_set = _workload(k, 23, 120, solid=2)
    res = _run(product, sets, gaps, gap_set, k, 2, **_OPT[opt])
    _check(product, sets, gaps, gap_set, res, k, 2, opt=opt, n_single=6)


def test_stream_restarts_per_gap(product):
    """a gap whose traceback draws (and whose choice depends on the values drawn) gives the same result first in the
    list, at position 500 and in the reversed list; the session's own stream is not advanced"""
    k = 31
    sets, gaps, gap_set = _workload(k, 41, 600)
    u = product.Graph.from_sets(sets, k, 1)
    sess = product.Session(u, 0, d_err=D_ERR, randseed=SEED)
    try:
        allg = [_gap(product, g) for g in gaps]
        base = sess.fill_sets(allg, gap_set)
        drawing = [i for i, r in enumerate(base) if r.draws > 1 and r.count > 1]
        assert drawing, "no gap with a traceback that has choices"
        t = drawing[0]
        others = [i for i in range(len(gaps)) if i != t][:500]
        for order in ([t] + others, others + [t], list(reversed(others + [t]))):
            res = sess.fill_sets([allg[i] for i in order], [gap_set[i] for i in order])
            assert _fields(res[order.index(t)]) == _fields(base[t])
        assert _sequence(gaps[t], base[t], False) == _oracle_sequence(sets[gap_set[t]], gaps[t], k, 1, {})
    finally:
        sess.destroy()
        u.free()
    # the list leaves the session's stream where it was: a single-set session filled after a set list draws from the seed
    gr = product.Graph.from_sets([sets[gap_set[t]]], k, 1)
    sess = product.Session(gr, 0, d_err=D_ERR, randseed=SEED)
    try:
        sess.fill_sets([_gap(product, gaps[t])], [0])
        assert _fields(sess.fill_batch([_gap(product, gaps[t])])[0]) == _fields(base[t])
    finally:
        sess.destroy()
        gr.free()


@pytest.mark.parametrize("env", [("G2S_RESIDENT", "1"), ("G2S_SEG_WAVES", "1"), ("G2S_SEG_WAVES", "2"),
                                 ("G2S_FORCE_SEGX", "1"), ("G2S_HOST_LOOKUP", "1")])
def test_switches_change_nothing(product, monkeypatch, env):
    k = 31
    sets, gaps, gap_set = _workload(k, 59, 300)
    base = _run(product, sets, gaps, gap_set, k, 1)
    with monkeypatch.context() as m:
        m.setenv(*env)
        res = _run(product, sets, gaps, gap_set, k, 1)
    for i in range(len(gaps)):
        assert _fields(res[i]) == _fields(base[i]), "gap %d" % i


def test_long_flanks_take_the_host_lookup(product):
    """flanks whose look-up text exceeds the kernel's staging buffer (G2S_FLANK_TEXT_MAX) resolve on the host, in
    the gap's own set"""
    k = 31
    sets, gaps, gap_set = _workload(k, 71, 12)
    genome = cases.toy_genome(71, 12000, k, repeats=6, tandem=2, snp_every=350)[0]
    fuz = 700
    pos, gl = 5000, 60
    big = dict(left=genome[pos - k - fuz:pos], right=genome[pos + gl:pos + gl + k + fuz], gap_len=gl + k, lmf=fuz,
               rmf=fuz, true_len=gl)
    assert (k + fuz) + 2 * (k + fuz) > 2048
    sets.append([genome[pos - 1200:pos + gl + 1200]])
    gaps.append(big)
    gap_set.append(len(sets) - 1)
    gaps.append(dict(big))
    gap_set.append(0)  # the same flanks in a set that does not hold them
    res = _run(product, sets, gaps, gap_set, k, 1)
    for i in range(len(gaps)):
        assert _sequence(gaps[i], res[i], False) == _oracle_sequence(sets[gap_set[i]], gaps[i], k, 1, {}), "gap %d" % i
    assert res[len(gaps) - 2].count > 0


def test_fill_sets_arguments(product):
    k = 31
    sets, gaps, gap_set = _workload(k, 83, 8)
    u = product.Graph.from_sets(sets, k, 1)
    sess = product.Session(u, 0, d_err=D_ERR, randseed=SEED)
    try:
        with pytest.raises(product.G2SError) as e:
            sess.fill_sets([_gap(product, gaps[0])], [len(sets)])
        assert e.value.code == -1
        g = gaps[1]
        with pytest.raises(product.G2SError) as e:
            sess.fill_sets([product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"], 3)], [0])
        assert e.value.code == -1
        with pytest.raises(product.G2SError) as e:  # several sets: only g2s_fill_sets knows which set a gap is in
            sess.fill_batch([_gap(product, gaps[0])])
        assert e.value.code == -1
    finally:
        sess.destroy()
        u.free()


def _canon(x):
    rc = x.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    code = str.maketrans("ACTG", "0123")  # GATB codec order A0 C1 T2 G3
    return min(x, rc, key=lambda y: y.translate(code))


def _set_view(product, u, s):
    """set s of a set graph as strings: {k-mer: (successors of both orientations, as strings)}"""
    first, cnt = u.set_nodes(s)
    out = {}
    for i in range(first, first + cnt):
        x = _canon(u.node_string(2 * i))  # (orientations are unitig-relative: the canonical string names the k-mer)
        v = u.set_node(s, x)
        assert v >> 1 == i and u.node_string(v) == x
        for w in u.successors(v) + u.successors(v ^ 1):
            assert first <= w >> 1 < first + cnt, "edge out of set %d" % s
        out[x] = ([u.node_string(w) for w in u.successors(v)], [u.node_string(w) for w in u.successors(v ^ 1)])
    return out


@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_set_build_equals_host_set_build(product, monkeypatch, capfd, k):
    """the keyed device build (dbg_gpu.hip) against the host build, set by set; sets with circular unitigs (a tandem
    read) in the middle, an empty set, a set of one copy at solid 2, overlapping sets"""
    sets, _, _ = _workload(k, 101 + k, 40, solid=2)
    rng = cases.SplitMix(k)
    unit = cases.random_dna(rng, k + 19)
    sets.insert(3, [unit * 4] * 2)               # one circular unitig
    sets.insert(7, [unit * 4, cases.random_dna(rng, 300)] * 2)
    sets.insert(9, [cases.random_dna(rng, 200)])  # every k-mer once: nothing solid at 2
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    dev = product.Graph.from_sets(sets, k, 2)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    assert "set graph build" in err and "on the GPU" in err, err[-2000:]
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    host = product.Graph.from_sets(sets, k, 2)
    try:
        assert dev.num_sets == host.num_sets == len(sets)
        assert dev.num_kmers == host.num_kmers and dev.num_unitigs == host.num_unitigs
        for s in range(len(sets)):
            assert dev.set_nodes(s) == host.set_nodes(s), "set %d" % s
            assert _set_view(product, dev, s) == _set_view(product, host, s), "set %d" % s
        assert dev.set_nodes(9)[1] == 0
        assert dev.validate() == (0, "")
    finally:
        dev.free()
        host.free()


@pytest.mark.parametrize("n_solid", [0, 1])
def test_device_set_build_with_no_or_one_solid_kmer(product, monkeypatch, capfd, n_solid):
    """the edges of the keyed build's scans (cases.barely_solid_reads): runs of (set, k-mer) and a total of zero behind
    the scan of their solid flags, and exactly one k-mer kept in one set; set by set against the host build"""
    k, solid = cases.BARELY_K, cases.BARELY_SOLID
    sets = [cases.barely_solid_reads(n_solid), cases.barely_solid_reads(0)[:1], []]
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    dev = product.Graph.from_sets(sets, k, solid)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    host = product.Graph.from_sets(sets, k, solid)
    try:
        if n_solid:
            assert "set graph build" in err and "on the GPU" in err, err[-2000:]
        else:  # (the device counted, found the union empty and handed it to the host build: it did run)
            assert "set graph on the host (size)" in err, err[-2000:]
        assert dev.num_sets == host.num_sets == len(sets)
        assert dev.num_kmers == host.num_kmers == n_solid and dev.num_unitigs == host.num_unitigs == n_solid
        for s in range(len(sets)):
            assert dev.set_nodes(s) == host.set_nodes(s) and dev.set_nodes(s)[1] == (n_solid if s == 0 else 0), "set %d" % s
            assert _set_view(product, dev, s) == _set_view(product, host, s), "set %d" % s
        assert dev.validate() == (0, "")
    finally:
        dev.free()
        host.free()
