"""Every k-mer width edge against the CPU oracle: k = 31/32 (64- to 128-bit words), 63/64 (128- to 256-bit) and 127 (the
widest).  Gap-by-gap fill parity over every kernel tier, resident lists at wide k, the flank look-ups at their own
limits (flank text per gap, the staged copy of long lists, right flanks longer than k + rmf, bytes other than ACGT) on
each path that does them, and the whole graph of the GPU build against the host build and the oracle's k-mer count."""
import random

import pytest

import cases
import pyref
from test_gpu_parity import _check_batch, _compare_with_oracle_in_parallel, _gaps, tier  # noqa: F401 (tier: fixture)

pytestmark = pytest.mark.gpu

LOOKUP_VARS = ("G2S_RESIDENT", "G2S_HOST_LOOKUP", "G2S_FORCE_SEGX", "G2S_NO_SEG_TIER", "G2S_HOST_BUILD",
               "G2S_DEBUG")


def _uneven_fuz(gaps, k, fuz):
    """lmf != rmf on most gaps: flanks cut down to k + lmf / k + rmf (lmf from the left end of the gap)"""
    out = []
    for i, g in enumerate(gaps):
        lmf, rmf = (fuz, (3 * i) % fuz) if i % 2 else ((5 * i) % fuz, fuz)
        lmf, rmf = min(lmf, g["lmf"]), min(rmf, g["rmf"])
        out.append(dict(g, left=g["left"][len(g["left"]) - (k + lmf):], right=g["right"][:k + rmf], lmf=lmf, rmf=rmf))
    return out


def _parity_fixture(k):
    """a 60 kbp toy genome (repeats, tandem arrays, a second haplotype with SNPs) with 40 gaps, and the hairpins and
    inversions of cases.strand_flip_genome (Q7 cases) with 20 more: 60 gaps, lmf != rmf on most"""
    seqs = cases.toy_genome(k + 300, 60000, k, repeats=12, tandem=3, snp_every=500)
    e = k + 20
    gaps = _uneven_fuz(cases.cut_gaps(k + 300, seqs[0], k, 10, 40, 20, 300, e), k, 10)
    fseqs, fgaps = cases.strand_flip_genome(k, 4000, k)
    assert any(g["lmf"] != g["rmf"] for g in gaps)
    return seqs + fseqs, gaps + fgaps, e


@pytest.mark.parametrize("k", [31, 32, 33, 63, 64, 65, 96, 127])
def test_fill_parity_at_every_width(product, oracle, tier, k):
    seqs, gaps, e = _parity_fixture(k)
    compared = filled = 0
    for skip, allp in ((False, True), (False, False), (True, True)):
        c, f, tm, _, _ = _check_batch(product, oracle, seqs, k, gaps, e, skip, allp)
        compared += c
        filled += f
        if tier == "res" and k % 2:  # (even k: the graph keeps a predecessor table, which resident mode does not take)
            assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (tm.resident_launches, tm.resident_fallbacks)
    assert compared >= 3 * 50 and filled >= 3 * 35, (compared, filled)


def _set(monkeypatch, **env):
    for v in LOOKUP_VARS:
        monkeypatch.delenv(v, raising=False)
    for a, b in env.items():
        monkeypatch.setenv(a, b)


@pytest.mark.parametrize("k,n", [(65, 300), (127, 600)])
def test_resident_lists_at_wide_k(product, oracle, monkeypatch, k, n):
    """resident mode at k >= 64: the look-up kernel runs in front of the fill kernel (inline_ok is false).  65 is the
    narrowest 256-bit width resident mode takes: at even k the graph keeps a predecessor table, which it does not"""
    seqs = cases.toy_genome(k + 400, 150000, k, repeats=20, tandem=4, snp_every=700)
    gaps = _uneven_fuz(cases.cut_gaps(k + 400, seqs[0], k, 10, n, 20, 250, 40), k, 10)
    _set(monkeypatch, G2S_RESIDENT="1")
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, k, gaps, 40)
    assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (tm.resident_launches, tm.resident_fallbacks)
    assert c >= n - 5 and f >= n // 2, (c, f)


def _long_list(product, oracle, monkeypatch, seqs, k, gaps, e, env, resident):
    _set(monkeypatch, **env)
    og = oracle.OracleGraph(seqs, k, 1)
    pg = product.Graph.from_seqs(seqs, k, 1)
    sess = product.Session(pg, 0, d_err=e, randseed=9)
    try:
        res, tm = sess.fill_batch(_gaps(product, gaps), True)
        if resident:
            assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (tm.resident_launches, tm.resident_fallbacks)
        else:
            assert tm.resident_launches == 0
        c, q7 = _compare_with_oracle_in_parallel(product, oracle, og, gaps, res, e, 9, threads=16)
        assert c + q7 == len(gaps) and c > len(gaps) - 10, (c, q7)
        assert sum(1 for r in res if r.count > 0) > len(gaps) // 2
    finally:
        sess.destroy()
        pg.free()
        og.free()


@pytest.mark.parametrize("k,env,resident", [(127, dict(G2S_RESIDENT="0"), False), (31, dict(G2S_RESIDENT="1"), True)])
def test_lists_of_2048_and_2049_valid_gaps(product, oracle, monkeypatch, k, env, resident):
    """upload_flanks copies descriptors and text to device memory once a list has more than 2048 valid gaps: at k = 127
    on the host path for the look-up kernel, at k = 31 in resident mode for the fill kernel's in-wave look-ups"""
    genome = cases.random_dna(cases.SplitMix(2048 + k), 400000)
    for n in (2048, 2049):
        gaps = _uneven_fuz(cases.cut_gaps(n + k, genome, k, 6, n, 10, 120, 20), k, 6)
        _long_list(product, oracle, monkeypatch, [genome], k, gaps, 20, env, resident)


# ---- the flank look-ups at their limits ------------------------------------------------------------------------------

_IUPAC = "NnRYKM"


def _flank_genome(k):
    seqs = cases.toy_genome(k + 500, 40000, k, repeats=6, snp_every=900)
    return seqs


def _cut(genome, rng, k, lmf, rmf, gl, e, left_extra="", right_extra=0, junk=False):
    """one gap of true length gl: flanks of k + lmf and k + rmf + right_extra characters (the extra ones from the genome,
    or random when junk), the left flank with left_extra characters behind it that fill_gap never reads"""
    pos = rng.randint(k + lmf + 10, len(genome) - gl - k - rmf - right_extra - 10)
    right = genome[pos + gl:pos + gl + k + rmf + right_extra]
    if junk and right_extra:
        right = right[:k + rmf] + cases.random_dna(rng, right_extra)
    claimed = gl + k + rng.choice([0, 0, e // 2, -e // 2, e])
    return dict(left=genome[pos - k - lmf:pos] + left_extra, right=right, gap_len=max(1, claimed), lmf=lmf, rmf=rmf)


def _text_size_lists(genome, k):
    """lists whose gaps carry (k + lmf) + 2 (k + rmf) = 2047, 2048 and 2049 bytes of flank text, one size a list"""
    rng = cases.SplitMix(7 * k)
    lists = []
    for size in (2047, 2048, 2049):
        gl = []
        for d in (1, 4, 9):  # lmf != rmf, lmf - rmf of several residues
            rmf = (size - 3 * k) // 3 - d
            lmf = size - 3 * k - 2 * rmf
            assert (k + lmf) + 2 * (k + rmf) == size and lmf != rmf
            gl.append(_cut(genome, rng, k, lmf, rmf, rng.randint(20, 200), 30))
        lists.append(("text%d" % size, gl))
    return lists


def _mark(s, rng, positions):
    s = list(s)
    for p in positions:
        s[p] = rng.choice(_IUPAC)
    return "".join(s)


def _shape_lists(genome, k):
    """right flanks exactly k + rmf long and 1, 2, 3 and 17 longer (the extra bases from the genome or random), left
    flanks longer than k + lmf, flanks in lower case or holding N, n, R, Y, K, M inside seed k-mers"""
    rng = cases.SplitMix(11 * k)
    shapes = []
    for extra in (0, 1, 2, 3, 17):
        for lmf, rmf in ((10, 3), (2, 10), (7, 0), (0, 7), (31, 30)):
            for junk in (False, True):
                left_extra = cases.random_dna(rng, extra)
                shapes.append(_cut(genome, rng, k, lmf, rmf, rng.randint(10, 150), 30, left_extra, extra, junk))
    odd = []
    for i in range(24):
        lmf, rmf = [(10, 10), (10, 4), (3, 10), (20, 1)][i % 4]
        g = _cut(genome, rng, k, lmf, rmf, rng.randint(10, 150), 30, right_extra=i % 3)
        if i % 6 == 0:
            g["left"], g["right"] = g["left"].lower(), g["right"].lower()
        elif i % 6 == 1:
            g["left"] = g["left"][:lmf + 2] + g["left"][lmf + 2:].lower()
        else:
            g["left"] = _mark(g["left"], rng, [rng.randint(0, k + lmf - 1) for _ in range(1 + i % 2)])
            g["right"] = _mark(g["right"], rng, [rng.randint(0, len(g["right"]) - 1) for _ in range(1 + i % 3)])
        odd.append(g)
    return [("shapes", shapes), ("bytes", odd)]


def _lookup_paths(k, name):
    paths = [("kernel", dict(G2S_RESIDENT="0")), ("host", dict(G2S_RESIDENT="0", G2S_HOST_LOOKUP="1"))]
    if k <= 63 and not name.startswith("text"):  # (lmf, rmf > 31 keep a list off the segment tier and resident mode)
        paths.append(("resident", dict(G2S_RESIDENT="1")))
    return paths


@pytest.mark.parametrize("k", [31, 63, 127])
def test_flank_lookup_edges(product, oracle, monkeypatch, k):
    seqs = _flank_genome(k)
    lists = _text_size_lists(seqs[0], k) + _shape_lists(seqs[0], k)
    og = oracle.OracleGraph(seqs, k, 1)
    pg = product.Graph.from_seqs(seqs, k, 1)
    try:
        for name, gl in lists:
            want = []
            rng = oracle.OracleRng(3)
            for g in gl:
                want.append(oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], 30, g["lmf"], g["rmf"]))
            assert any(o.count > 0 for o in want), name
            for path, env in _lookup_paths(k, name):
                _set(monkeypatch, **env)
                sess = product.Session(pg, 0, d_err=30, randseed=3)
                try:
                    res, tm = sess.fill_batch(_gaps(product, gl), True)
                finally:
                    sess.destroy()
                if path == "resident":
                    assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (name, tm.resident_launches)
                for i, (r, o) in enumerate(zip(res, want)):
                    what = "%s gap %d on the %s path" % (name, i, path)
                    if o.info.q7:
                        assert r.flags & product.G2S_GAP_Q7, what
                        break  # (the rand() streams may part here; the lists hold few Q7 cases)
                    assert r.count == o.count and r.draws == o.info.draws, (what, r.count, o.count, r.draws, o.info.draws)
                    assert r.phaseC_count == o.info.phaseC_count and r.lengths == o.lengths, what
                    if o.phase_d:
                        assert (r.left_fuz, r.right_fuz, r.fill) == (o.left_fuz, o.right_fuz, o.fill), what
                        assert r.substats == o.substats, what
    finally:
        pg.free()
        og.free()


# ---- the whole graph ---------------------------------------------------------------------------------------------------

def _build_reads(k):
    """coverage 3 from 300 bp reads, some reads eight times over, N runs, lower case, reads shorter than k"""
    rr = random.Random(1000 + k)
    genome = "".join(rr.choice("ACGT") for _ in range(6000))
    reads = []
    for i in range(0, len(genome) - 300, 100):
        r = genome[i:i + 300]
        if i % 700 == 0:
            r = r[:120] + "NNNNN" + r[125:]
        if i % 500 == 0:
            r = r[:40] + r[40:200].lower() + r[200:]
        reads.append(r)
        if i % 1100 == 0:
            reads += [r] * 7
    reads += [genome[50:50 + max(1, k - 1)], genome[900:900 + max(1, k // 2)], "n" * (k + 3)]
    return reads


def _graph_map(g):
    """every oriented node: string -> (successor strings, predecessor strings), GATB order"""
    out = {}
    for v in range(2 * g.num_kmers):
        s = g.node_string(v)
        w = g.node(s)
        if s == pyref.revcomp(s):  # a palindrome (even k): both ids spell it; the one node() gives carries the edges
            assert w in (v, v ^ 1), (v, s)
        else:
            assert w == v and s not in out, (v, s)
        if w == v:
            out[s] = (tuple(g.node_string(x) for x in g.successors(v)), tuple(g.node_string(x) for x in g.predecessors(v)))
    return out


@pytest.mark.parametrize("k", [1, 2, 11, 12, 13, 31, 32, 33, 63, 64, 65, 127])
def test_graph_build_whole_graph(product, oracle, monkeypatch, capfd, k):
    """every node of the GPU build against the host build (G2S_HOST_BUILD=1), by string: node ids may differ.  Below
    k = 12 the prefix index is 2k bits wide, from 12 on 22 bits."""
    reads = _build_reads(k)
    for solid in (1, 2, 3):
        _set(monkeypatch, G2S_HOST_BUILD="1")
        gh = product.Graph.from_seqs(reads, k, solid)
        _set(monkeypatch, G2S_DEBUG="1")
        capfd.readouterr()
        gg = product.Graph.from_seqs(reads, k, solid)
        err = capfd.readouterr().err
        _set(monkeypatch)
        og = oracle.OracleGraph(reads, k, solid)
        try:
            assert "GPU sort" in err, err[-2000:]
            assert gg.num_kmers == gh.num_kmers == og.num_kmers > 0, (solid, gg.num_kmers, gh.num_kmers, og.num_kmers)
            assert gg.num_unitigs == gh.num_unitigs
            assert gg.validate() == (0, "") and gh.validate() == (0, "")
            mg, mh = _graph_map(gg), _graph_map(gh)
            assert mg == mh, solid
            p = pyref.Graph(reads, k, solid)
            assert {pyref.canon(s)[0] for s in mg} == p.kmers, solid
            for s, (succ, pred) in mg.items():
                assert list(succ) == p.succ(s) and list(pred) == p.pred(s), s
        finally:
            gg.free()
            gh.free()
            og.free()


@pytest.mark.parametrize("n_solid", [0, 1])
def test_graph_build_with_no_or_one_solid_kmer(product, monkeypatch, capfd, n_solid):
    """the edges of the device build's scans (cases.barely_solid_reads): run heads and a total of zero behind the scan
    of their solid flags, so nothing to compact; and one k-mer kept, whose tables are scans over two elements.  Every
    node against the host build."""
    reads, k, solid = cases.barely_solid_reads(n_solid), cases.BARELY_K, cases.BARELY_SOLID
    _set(monkeypatch, G2S_HOST_BUILD="1")
    gh = product.Graph.from_seqs(reads, k, solid)
    _set(monkeypatch, G2S_DEBUG="1")
    capfd.readouterr()
    gg = product.Graph.from_seqs(reads, k, solid)
    err = capfd.readouterr().err
    _set(monkeypatch)
    try:
        assert "GPU sort" in err, err[-2000:]
        if n_solid:  # (an empty graph has no tables to make)
            assert any("tables, unitig order, id space:" in ln and ln.endswith("on the GPU") for ln in err.splitlines()), err[-2000:]
        assert gg.num_kmers == gh.num_kmers == n_solid and gg.num_unitigs == gh.num_unitigs == n_solid
        assert gg.validate() == (0, "") and gh.validate() == (0, "")
        assert _graph_map(gg) == _graph_map(gh) and len(_graph_map(gg)) == 2 * n_solid
    finally:
        gg.free()
        gh.free()
