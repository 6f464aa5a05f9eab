"""Even k on the segment tier and in resident mode: the back-record table the kernels walk backwards with on a graph
that has an explicit predecessor table (seg_tables.h), and fills of gaps whose paths run through palindromic k-mers
(tests/even_k_fill_cases.py) on every path a list can take, gap by gap against the oracle.  Every run asserts the path it
names: before even-k graphs were admitted to the segment tier these lists ran on the HBM tier, whatever was asked."""
import pytest

import even_k_cases
import even_k_fill_cases as E
import pyref
from test_gpu_parity import _check_batch, _gaps, _result_tuple

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
PATH_VARS = ("G2S_RESIDENT", "G2S_SEG_WAVES", "G2S_FORCE_SEGX", "G2S_DEVICE_D2", "G2S_NO_SEG_TIER",
             "G2S_HOST_BUILD", "G2S_NO_SEGX_TIER", "G2S_HOST_D2")
PATHS = ("host", "resident", "waves1", "waves2", "segx", "resident_d2")


def _set_path(monkeypatch, path):
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    if path == "default":
        return
    monkeypatch.setenv("G2S_RESIDENT", "1" if path.startswith("resident") else "0")
    if path in ("waves1", "waves2"):
        monkeypatch.setenv("G2S_SEG_WAVES", path[-1])
    elif path == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")
    elif path == "resident_d2":
        monkeypatch.setenv("G2S_DEVICE_D2", "1")
    elif path == "hbm":  # what every even-k list ran on before
        monkeypatch.setenv("G2S_NO_SEG_TIER", "1")


def _check_path(path, tm, n):
    what = (path, tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps, tm.retried_gaps, tm.resident_launches, tm.resident_fallbacks)
    if path == "hbm":
        assert tm.seg_tier_gaps == 0 and tm.segx_tier_gaps == 0 and tm.lds_tier_gaps == 0 and tm.resident_launches == 0, what
        return
    assert tm.seg_tier_gaps == n or tm.segx_tier_gaps > 0, what
    assert tm.lds_tier_gaps == 0 and tm.retried_gaps == 0, what
    if path.startswith("resident") or path == "default":
        assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, what
    else:
        assert tm.resident_launches == 0, what
    if path == "segx":
        assert tm.segx_tier_gaps > 0 and tm.seg_tier_gaps == 0, what


# ---- 1. the back records ----------------------------------------------------------------------------------------------

def _check_back_records(product, g, reads, k):
    p = pyref.Graph(reads, k, 1)
    n2 = 2 * g.num_kmers
    strs = [g.node_string(v) for v in range(n2)]
    live = [g.node(strs[v]) == v for v in range(n2)]  # (not live: the strand of a palindrome that does not exist)
    pal = lambda s: s == pyref.revcomp(s)  # noqa: E731
    # the unitig-internal edge into s, if there is one (dbg.cpp: unitig_order's step — one way out of u, one way into s,
    # two k-mers, and no palindrome at either end: a palindrome is a unitig of its own)
    prev = {}
    for v in range(n2):
        s = strs[v]
        if not live[v]:
            continue
        pr = p.pred(s)
        u = pr[0] if len(pr) == 1 else None
        if u is not None and (p.succ(u) != [s] or pyref.canon(u)[0] == pyref.canon(s)[0] or pal(u) or pal(s)):
            u = None
        prev[s] = u
    palindromes = 0
    for v in range(n2):
        words, rem = product.test_seg_back_record(g, 0, v)
        s = strs[v]
        if not live[v]:  # a palindrome's missing strand: the palindrome's own predecessors, no step
            assert pal(s) and rem == 0, (v, s, rem)
            b = s
        else:
            steps, cur, circular = 0, s, False
            while prev[cur] is not None:
                cur = prev[cur]
                steps += 1
                if cur == s:
                    circular = True
                    break
            far = v - 2 * rem if v % 2 == 0 else v + 2 * rem  # back from an even id the ids shrink
            assert 0 <= far < n2, (v, rem)
            if circular:  # the numbering cuts a circular unitig somewhere: the walk ends there, in front of a full turn
                assert rem < steps, (v, s, rem, steps)
                b = strs[far]
            else:
                assert rem == steps, (v, s, rem, steps)
                b = cur
                assert strs[far] == b, (v, s, rem)
        palindromes += pal(b)
        got = []
        for slot, w in enumerate(words):
            if w != INVALID:
                ps = strs[w ^ 1]
                assert live[w ^ 1] and ps[0] == "TGAC"[slot] and ps[1:] == b[:-1], (v, s, slot, ps)  # GATB's predecessor order
                got.append(ps)
        assert got == p.pred(b), (v, s, b, got, p.pred(b))
    return palindromes


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("k", [4, 12, 32, 64])
def test_back_records_are_pyrefs_predecessors(product, monkeypatch, k, build):
    _set_path(monkeypatch, "default")
    if build == "host":
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
    reads, designed = even_k_cases.designed_reads(k, 1)
    g = product.Graph.from_seqs(reads, k, 1)
    try:
        assert _check_back_records(product, g, reads, k) >= len(set(designed.values()))
    finally:
        g.free()


def test_back_record_at_odd_k_is_the_forward_record_of_the_other_strand(product, monkeypatch):
    """no table of its own at odd k (predecessors(b)[i] = succ(b ^ 1)[i] ^ 1): the records are pyref's predecessors all the
    same, and the segment tables add rem (8 bytes a k-mer) and urec (64) to the uploaded graph, nothing else; at even k
    the back records are 64 bytes a k-mer more"""
    _set_path(monkeypatch, "default")
    reads, _ = even_k_cases.designed_reads(12, 1)
    for k, table_bytes in ((11, 8 + 64), (12, 8 + 64 + 64)):
        g = product.Graph.from_seqs(reads, k, 1)
        try:
            g.upload(0)
            uploaded = g.device_bytes(0)  # before the first hook call, which builds the tables
            assert uploaded > 0
            palindromes = _check_back_records(product, g, reads, k)
            assert (palindromes > 0) == (k == 12)
            assert g.device_bytes(0) == uploaded + g.num_kmers * table_bytes, (k, uploaded, g.device_bytes(0), g.num_kmers)
            sess = product.Session(g, 0, d_err=E.D_ERR, randseed=5)  # a session finds the tables there
            sess.destroy()
            assert g.device_bytes(0) == uploaded + g.num_kmers * table_bytes, k
        finally:
            g.free()


# ---- 2. parity on every path ------------------------------------------------------------------------------------------

def _outcomes(oracle, reads, gaps, k, allp):
    from test_even_k_fill_cases import oracle_outcomes
    return oracle_outcomes(oracle, reads, gaps, k, allp)


# (-best-only on the host's and on the device's traceback; the other paths share one of the two)
@pytest.mark.parametrize("path,allp", [(p, True) for p in PATHS] + [("host", False), ("resident", False)])
@pytest.mark.parametrize("k", E.K)
def test_designed_lists_equal_the_oracle_on_every_path(product, oracle, monkeypatch, k, path, allp):
    _set_path(monkeypatch, path)
    reads, gaps = E.build(k)
    E.class_condition(gaps, _outcomes(oracle, reads, gaps, k, allp))
    compared, filled, tm, _, _ = _check_batch(product, oracle, reads, k, gaps, E.D_ERR, allp=allp)
    _check_path(path, tm, len(gaps))
    assert filled >= len(E.CLASSES) and compared < len(gaps)  # (some gap is the oracle's Q7 case: flagged, not compared)


# ---- 3. the HBM tier, on which even k ran before, against the segment tier ---------------------------------------------

def _fill(product, monkeypatch, path, g, gaps, allp=True):
    _set_path(monkeypatch, path)
    sess = product.Session(g, 0, d_err=E.D_ERR, all_paths=allp, randseed=5)
    try:
        res, tm = sess.fill_batch(_gaps(product, gaps), True)
        return [_result_tuple(r) for r in res], tm
    finally:
        sess.destroy()


@pytest.mark.parametrize("k", E.K)
def test_segment_tier_equals_the_hbm_tier(product, monkeypatch, k):
    reads, gaps = E.build(k)
    _set_path(monkeypatch, "default")
    g = product.Graph.from_seqs(reads, k, 1)
    try:
        old, tm = _fill(product, monkeypatch, "hbm", g, gaps)
        _check_path("hbm", tm, len(gaps))
        for path in ("host", "resident"):
            new, tm = _fill(product, monkeypatch, path, g, gaps)
            _check_path(path, tm, len(gaps))
            for i, (a, b) in enumerate(zip(old, new)):
                assert a == b, (path, i, gaps[i]["cls"])
    finally:
        g.free()


# ---- 4. the default threshold ------------------------------------------------------------------------------------------

def test_a_list_over_256_gaps_runs_resident_by_default(product, oracle, monkeypatch):
    _set_path(monkeypatch, "default")
    reads, gaps = E.padded(32)
    assert len(gaps) > 256
    compared, filled, tm, _, _ = _check_batch(product, oracle, reads, 32, gaps, E.D_ERR)
    _check_path("default", tm, len(gaps))
    assert filled > 150


# ---- 5. set lists --------------------------------------------------------------------------------------------------------

def test_set_list_on_an_even_k_set_graph_runs_resident(product, monkeypatch):
    k = 32
    reads, gaps = E.build(k)
    # one set per gap of the classes a and d: the reads that hold the gap's flanks (its island, both haplotypes of it)
    chosen = [g for g in gaps if g["cls"] in "ad"]
    set_lists = [[j for j, r in enumerate(reads) if g["left"] in r or g["right"] in r] for g in chosen]
    assert len(chosen) >= 8 and all(set_lists) and any(len(s) == 2 for s in set_lists)
    _set_path(monkeypatch, "default")
    want = []
    for g, lst in zip(chosen, set_lists):  # the gap in the graph of its own reads, from a fresh srand
        sg = product.Graph.from_seqs([reads[j] for j in lst], k, 1)
        try:
            res, _ = _fill(product, monkeypatch, "host", sg, [g])
            want.append(res[0])
        finally:
            sg.free()
    _set_path(monkeypatch, "resident")
    pg = product.Graph.from_pool(reads, set_lists, k, 1)
    sess = product.Session(pg, 0, d_err=E.D_ERR, randseed=5)
    try:
        assert pg.num_sets == len(chosen)
        res, tm = sess.fill_sets(_gaps(product, chosen), list(range(len(chosen))), True)
        assert [_result_tuple(r) for r in res] == want
        assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (tm.resident_launches, tm.resident_fallbacks)
        assert sum(1 for r in res if r.count > 0) >= len(chosen) - 2
    finally:
        sess.destroy()
        pg.free()


# ---- 6. a saved graph ------------------------------------------------------------------------------------------------------

def test_saved_even_k_graph_fills_on_the_segment_tier(product, monkeypatch, tmp_path):
    k = 32
    reads, gaps = E.build(k)
    _set_path(monkeypatch, "default")
    g = product.Graph.from_seqs(reads, k, 1)
    try:
        want, tm = _fill(product, monkeypatch, "host", g, gaps)
        _check_path("host", tm, len(gaps))
        g.save(str(tmp_path / "even.g2s"))
    finally:
        g.free()
    g2 = product.Graph.load(str(tmp_path / "even.g2s"))
    try:
        got, tm = _fill(product, monkeypatch, "host", g2, gaps)
        assert got == want and tm.seg_tier_gaps > 0
        _check_path("host", tm, len(gaps))
    finally:
        g2.free()
