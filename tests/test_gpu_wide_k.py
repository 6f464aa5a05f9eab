"""k-mer lengths 64 to 127 on the GPU: the graph build with 256-bit keys (dbg_gpu.hip) against the host build, and the
fill of gap lists at such k against the string restatement of the reference (oracle/pyref.py): FASTA byte for byte,
the per-gap log lines, on every path a list can take (the flank look-ups go through the look-up kernel at k >= 64)."""
import os
import random
import re
import subprocess

import pytest

import cases
import pyref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-core")
D_ERR, FUZ, SEED = 100, 10, 1
PATH_VARS = ("G2S_RESIDENT", "G2S_SEG_WAVES", "G2S_FORCE_SEGX", "G2S_HOST_BUILD", "G2S_DEBUG")


def _gap_lines(log):
    """the per-gap lines and the summary (pyref does not print the parameter echo in front of them)"""
    return [ln for ln in log.splitlines() if ln.startswith(("Scaffold:", "SubgraphStats:")) or re.match(r"Filled \d+ gaps out of \d+$", ln)]


def _fixture(k):
    seqs = cases.toy_genome(k, 20000, k, repeats=25, tandem=3, snp_every=400)
    gl = cases.cut_gaps(k, seqs[0], k, FUZ, 40, 50, 400, D_ERR)
    records = [("g%d" % i, g["left"] + "N" * g["gap_len"] + g["right"]) for i, g in enumerate(gl)]
    return seqs, records


def _scaffolds_text(records):
    return "".join(">%s\n%s\n" % r for r in records)


def _pyref(monkeypatch, seqs, records, k, **kw):
    """pyref's (FASTA, log, filled, gaps); no gap may have met both strands of a k-mer (Q7)"""
    infos = []

    class _Info(pyref.Info):
        def __init__(self):
            super().__init__()
            infos.append(self)

    with monkeypatch.context() as m:
        m.setattr(pyref, "Info", _Info)
        out = pyref.execute_scaffolds(pyref.Graph(seqs, k, 1), records, k, D_ERR, FUZ, SEED, **kw)
    assert infos and not any(i.q7 for i in infos)
    return out


def _graph(product, monkeypatch, capfd, seqs, k, solid=1):
    """the GPU build, asserting that the k-mer set was sorted on the device"""
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    g = product.Graph.from_seqs(seqs, k, solid)
    monkeypatch.delenv("G2S_DEBUG")
    err = capfd.readouterr().err
    assert "GPU sort" in err, err[-2000:]
    return g


def _set_path(monkeypatch, path):
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("G2S_RESIDENT", "1" if path == "resident" else "0")
    if path in ("waves1", "waves2"):
        monkeypatch.setenv("G2S_SEG_WAVES", path[-1])
    elif path == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")


def _check_path(path, tm):
    if path == "resident":
        assert tm.resident_launches >= 1 and tm.resident_fallbacks == 0, (tm.resident_launches, tm.resident_fallbacks)
    else:
        assert tm.resident_launches == 0
    if path == "segx":
        assert tm.segx_tier_gaps > 0 and tm.seg_tier_gaps == 0, (tm.seg_tier_gaps, tm.segx_tier_gaps)
    elif path in ("waves1", "waves2"):
        assert tm.seg_tier_gaps > 0, tm.seg_tier_gaps


def _run(product, g, text, k, **kw):
    sess = product.Session(g, 0, d_err=D_ERR, randseed=SEED, **kw)
    try:
        fa, log, gaps, filled = sess.execute_scaffolds(text, k, solid=1, max_fuz=FUZ)
        return fa, log, gaps, filled, sess.last_timing()
    finally:
        sess.destroy()


def _wide_reads(k):
    rr = random.Random(k)
    genome = "".join(rr.choice("ACGT") for _ in range(30000))
    reads = []
    for i in range(0, len(genome) - 400, 150):  # 400 bp reads every 150 bp: coverage 2-3
        r = genome[i:i + 400]
        if i % 900 == 0:
            r = r[:200] + "N" + r[201:]
        if i % 1350 == 0:
            r = r.lower()
        reads.append(r)
    reads.append(genome[:k - 1])  # shorter than k: contributes nothing
    return genome, reads


@pytest.mark.parametrize("k", [65, 96, 101, 127])
def test_gpu_graph_build_at_wide_k_equals_host_build(product, monkeypatch, capfd, k):
    genome, reads = _wide_reads(k)
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    gh = product.Graph.from_seqs(reads, k, 2)
    gg = _graph(product, monkeypatch, capfd, reads, k, solid=2)
    try:
        assert gg.num_kmers == gh.num_kmers and gg.num_kmers > 15000
        assert gg.num_unitigs == gh.num_unitigs
        assert gg.validate() == (0, "")
        rr = random.Random(k + 1)
        for _ in range(400):
            p = rr.randrange(0, len(genome) - k)
            km = genome[p:p + k]
            a, b = gg.node(km), gh.node(km)
            assert (a == 0xFFFFFFFF) == (b == 0xFFFFFFFF)
            if a != 0xFFFFFFFF:
                assert gg.node_string(a) == km and gh.node_string(b) == km
                assert gg.node_string(a ^ 1) == gh.node_string(b ^ 1)
                assert [gg.node_string(x) for x in gg.successors(a)] == [gh.node_string(x) for x in gh.successors(b)]
                assert [gg.node_string(x) for x in gg.predecessors(a)] == [gh.node_string(x) for x in gh.predecessors(b)]
    finally:
        gg.free()
        gh.free()


_PATHS = {65: ("host", "resident", "waves1", "waves2", "segx"), 101: ("host", "resident"), 127: ("host", "waves2")}


@pytest.mark.parametrize("k", [65, 101, 127])
def test_fill_at_wide_k_equals_pyref_on_every_path(product, monkeypatch, capfd, tmp_path, k):
    seqs, records = _fixture(k)
    text = _scaffolds_text(records)
    pfa, plog, pfilled, pgaps = _pyref(monkeypatch, seqs, records, k)
    assert pgaps == 40 and 10 <= pfilled < 40
    g = _graph(product, monkeypatch, capfd, seqs, k)
    try:
        for path in _PATHS[k]:
            _set_path(monkeypatch, path)
            fa, log, gaps, filled, tm = _run(product, g, text, k)
            assert (gaps, filled) == (pgaps, pfilled), path
            assert fa == pfa, path
            assert _gap_lines(log) == _gap_lines(plog), path
            _check_path(path, tm)
    finally:
        g.free()
    if k != 101:
        return
    # the command line as a drop-in, with the argv of the reference's wrapper
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    reads, scaf, out = tmp_path / "reads.fa", tmp_path / "scaf.fa", tmp_path / "out.fa"
    reads.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    scaf.write_text(text)
    res = subprocess.run([CORE, "-k", str(k), "-fuz", str(FUZ), "-solid", "1", "-nb-cores", "1", "-dist-error", str(D_ERR),
                          "-max-mem", "20", "-randseed", str(SEED), "-reads", str(reads), "-filled", str(out),
                          "-scaffolds", str(scaf)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert out.read_text() == pfa
    assert _gap_lines(res.stdout) == _gap_lines(plog)


def test_fill_options_and_multi_gap_record_at_wide_k(product, monkeypatch, capfd):
    """-all-upper, -best-only, -unique and one scaffold record with several gaps, at k = 65"""
    k = 65
    seqs, records = _fixture(k)
    text = _scaffolds_text(records)
    g = _graph(product, monkeypatch, capfd, seqs, k)
    try:
        _set_path(monkeypatch, "host")
        for opt, pkw, skw in (("all-upper", dict(skip_confident=True), dict(skip_confident=True)),
                              ("best-only", dict(all_paths=False), dict(all_paths=False)),
                              ("unique", dict(unique=True), dict(unique_paths=True))):
            pfa, plog, pfilled, pgaps = _pyref(monkeypatch, seqs, records, k, **pkw)
            fa, log, gaps, filled, _ = _run(product, g, text, k, **skw)
            assert (gaps, filled) == (pgaps, pfilled), opt
            assert fa == pfa, opt
            assert _gap_lines(log) == _gap_lines(plog), opt
        genome = seqs[0]
        rec = ("multi", cases.scaffold_record(genome, k, FUZ, [(1000 + 1500 * j, 60 + 7 * j, 60 + 7 * j + 3) for j in range(8)]))
        pfa, plog, pfilled, pgaps = _pyref(monkeypatch, seqs, [rec], k)
        assert pgaps == 8 and pfilled > 0
        for path in ("host", "resident"):
            _set_path(monkeypatch, path)
            fa, log, gaps, filled, tm = _run(product, g, _scaffolds_text([rec]), k)
            assert (gaps, filled, fa) == (pgaps, pfilled, pfa), path
            assert _gap_lines(log) == _gap_lines(plog), path
            _check_path(path, tm)
    finally:
        g.free()


def test_single_gap_command_line_at_k127(product, monkeypatch, tmp_path):
    k = 127
    seqs, _ = _fixture(k)
    gl = cases.cut_gaps(k, seqs[0], k, FUZ, 40, 50, 400, D_ERR)
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    reads = tmp_path / "reads.fa"
    reads.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    G = pyref.Graph(seqs, k, 1)
    filled = []
    for i in (0, 2, 5):  # (flanks of k + 10: 2 paths, none, 20 paths)
        left, right, length = gl[i]["left"], gl[i]["right"], gl[i]["gap_len"]
        assert len(left) == len(right) == k + FUZ
        cnt, lf, rf, fill, sub = pyref.fill_gap(G, pyref.GlibcRand(SEED), left, right, length, D_ERR, FUZ, FUZ, False, True,
                                                True, pyref.Info())
        want = left[:len(left) - lf] + pyref.fill_string(fill, FUZ - lf) if cnt > 0 else left + "N" * length + right
        filled.append(cnt > 0)
        out = tmp_path / ("single%d.fa" % i)
        res = subprocess.run([CORE, "-k", str(k), "-fuz", str(FUZ), "-solid", "1", "-dist-error", str(D_ERR), "-randseed",
                              str(SEED), "-reads", str(reads), "-filled", str(out), "-left", left, "-right", right,
                              "-length", str(length)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        lines = out.read_text().splitlines()
        assert len(lines) == 2 and lines[0].startswith(">") and lines[1] == want, (i, cnt)
        tail = pyref.fill_string(fill, FUZ - lf) if fill is not None else ""
        want_log = pyref.stats_line("", len(left) - FUZ - lf, len(left), len(left) + length, cnt, tail, k, FUZ, FUZ, lf, rf,
                                    False, False, sub, length)
        assert _gap_lines(res.stdout) == want_log.splitlines(), (i, cnt)
    assert filled == [True, False, True]


def test_c2_shaped_list_at_k127(product, oracle, monkeypatch, capfd):
    """at size: the GPU graph equals the host graph; the host path, resident mode and the segment tier on one and on
    two waves give identical results, nothing falls back to the host, and the host path's FASTA and per-gap lines are
    the CPU oracle's"""
    k = 127
    reads = product.G2S.synth_genome(3_000_000, 3, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    scaf = product.G2S.synth_gaps(reads, k, 10, 500, 200, 1000, 20240103)
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    gh = product.Graph.from_seqs(seqs, k, 1)
    gg = _graph(product, monkeypatch, capfd, seqs, k)
    try:
        assert (gg.num_kmers, gg.num_unitigs) == (gh.num_kmers, gh.num_unitigs)
        rr = random.Random(5)
        for _ in range(300):
            s = seqs[rr.randrange(len(seqs))]
            p = rr.randrange(0, len(s) - k)
            a, b = gg.node(s[p:p + k]), gh.node(s[p:p + k])
            assert gg.node_string(a) == gh.node_string(b) == s[p:p + k]
            assert [gg.node_string(x) for x in gg.successors(a)] == [gh.node_string(x) for x in gh.successors(b)]
        gh.free()
        gh = None
        outs = {}
        for path in ("host", "resident", "waves1", "waves2"):
            _set_path(monkeypatch, path)
            sess = product.Session(gg, 0, d_err=500, randseed=1)
            try:
                fa, log, gaps, filled = sess.execute_scaffolds(scaf, k, solid=1, max_fuz=10)
                tm = sess.last_timing()
            finally:
                sess.destroy()
            assert gaps == 500 and filled > 0, (path, filled)
            _check_path(path, tm)
            outs[path] = (fa, _gap_lines(log))
        assert all(o == outs["host"] for o in outs.values())
        og = oracle.OracleGraph(seqs, k, 1)
        try:
            assert og.num_kmers == gg.num_kmers
            ofa, olog, sm = oracle.execute_scaffolds(og, scaf, k, solid=1, d_err=500, max_fuz=10, randseed=1)
        finally:
            og.free()
        assert sm.gaps == 500 and sm.q7_gaps == 0
        assert outs["host"] == (ofa, _gap_lines(olog))
    finally:
        gg.free()
        if gh is not None:
            gh.free()
