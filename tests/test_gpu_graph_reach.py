"""A single graph bounded to its gap list's reach, on the device (gap2seq_amd/csrc/graph_reach.h): the device build
against the host build node for node on the cases of tests/test_graph_reach.py and on frontiers wider than a workgroup,
through the key-range passes, from read files, with a queue that has to grow; fills on the bounded graph against fills
on the whole one; the cap; the command line."""
import gzip
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import cases  # noqa: E402
import graph_reach_cases as GC  # noqa: E402
import reach_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

CORE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-core")
TOO_MANY = "too many k-mers for 32-bit oriented node ids"
SEED = 1


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("G2S_HOST_BUILD", "G2S_BUILD_MAX_KMERS", "G2S_BUILD_REACH", "G2S_BUILD_PASS_KEYS", "G2S_REACH_QUEUE_CAP"):
        monkeypatch.delenv(name, raising=False)


def _host(P, monkeypatch, build):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    try:
        g = build()
        assert P.test_last_graph_reach()["on_device"] == 0
        return g
    finally:
        monkeypatch.delenv("G2S_HOST_BUILD")


def _both(P, monkeypatch, build, passes=None):
    """build() on the device and on the host: the same graph, node for node.  Returns the device build's record."""
    dev = build()
    info = P.test_last_graph_reach()
    host = _host(P, monkeypatch, build)
    hinfo = P.test_last_graph_reach()
    try:
        assert info["on_device"] == 1, info
        assert dev.bounded and dev.validate() == (0, "")
        GC.assert_same_graph(dev, host)
        for key in ("records", "seeds", "seeds_in_full", "full_kmers", "kept_kmers"):
            assert info[key] == hinfo[key], key
        if passes is not None:
            assert info["passes"] >= passes
    finally:
        dev.free()
        host.free()
    return info


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", GC.KS)
def test_the_device_build_equals_the_host_build(product, monkeypatch, k, solid):
    seqs, gaps = GC.workload(k, solid)
    for name, records in GC.scenarios(k, gaps).items():
        reach = GC.reach_of(product, records)
        info = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, solid, reach=reach))
        assert 0 < info["kept_kmers"] < info["full_kmers"], name
    for records in ([(gaps["D"], 5)], []):   # no seed in the graph, no record: empty
        reach = GC.reach_of(product, records)
        info = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, solid, reach=reach))
        assert info["kept_kmers"] == 0


@pytest.mark.parametrize("k,r", [(4, 2), (32, 7), (64, 7)])
def test_a_palindrome_on_the_rim(product, monkeypatch, k, r):
    seqs, gap, pal = GC.palindrome_case(k, r)
    for radius in (r - 1, r, r + 1):
        full, kept = GC.model(seqs, [(gap, radius)], k, 1)
        assert (pal in kept) == (radius >= r)
        u = product.Graph.from_seqs(seqs, k, 1, reach=[(GC.gap_obj(product, gap), radius)])
        try:
            assert product.test_last_graph_reach()["on_device"] == 1
            GC.assert_matches_model(product, u, full, kept)
        finally:
            u.free()


def _many_records(k, n, length, seed):
    """n records spread over a random genome of `length` bases: (seqs, records) with radii 0 .. 24"""
    rng = cases.SplitMix(seed)
    genome = cases.random_dna(rng, length)
    step = (length - 4 * k - 200) // n
    records = []
    for i in range(n):
        pos = k + 20 + i * step
        g = dict(left=genome[pos - k - 2:pos], right=genome[pos + 12:pos + 12 + k + 2], gap_len=12 + k, lmf=2, rmf=2)
        records.append((g, (i * 7) % 25))
    return [genome, cases.random_dna(rng, 400)], records


def test_300_records_a_frontier_wider_than_a_workgroup(product, monkeypatch):
    k = 31
    seqs, records = _many_records(k, 300, 40000, 11)
    reach = GC.reach_of(product, records)
    info = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach))
    assert info["records"] == 300 and info["seeds_in_full"] >= 300 * 8 > 256   # (2 700 seeds; from level 24 on every record's frontier is live)
    assert 0 < info["kept_kmers"] < info["full_kmers"]
    full, kept = GC.model(seqs, records, k, 1)
    assert info["kept_kmers"] == len(kept) and info["full_kmers"] == len(full)


def test_a_single_path_of_12_kbp(product, monkeypatch):
    """one read, one path: the kept set is the stretches within the radii of the flanks.  The first two records enter
    together and their balls meet 101 levels later at one k-mer (the first's right edge starts at 541 + L, the second's
    left edge at 777 - 34 - L): two frontier k-mers share a neighbour, and one claim wins"""
    k = 33
    rng = cases.SplitMix(5)
    path = cases.random_dna(rng, 12000)
    records = []
    for pos, radius in ((500, 120), (777, 120), (6000, 300), (11000, 0)):
        records.append((dict(left=path[pos - k - 1:pos], right=path[pos + 40:pos + 40 + k + 1], gap_len=40 + k, lmf=1, rmf=1), radius))
    reach = GC.reach_of(product, records)
    info = _both(product, monkeypatch, lambda: product.Graph.from_seqs([path], k, 1, reach=reach))
    full, kept = GC.model([path], records, k, 1)
    assert info["kept_kmers"] == len(kept) and info["full_kmers"] == len(full) == 12000 - k + 1
    assert 0 < len(kept) < len(full) and info["levels"] == 300


def test_the_table_from_key_range_passes(product, monkeypatch):
    k = 31
    seqs, records = _many_records(k, 40, 9000, 12)
    reach = GC.reach_of(product, records)
    whole = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach))
    assert whole["passes"] == 0
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", "2500")
    info = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach), passes=3)
    assert info["kept_kmers"] == whole["kept_kmers"] and info["full_kmers"] == whole["full_kmers"]
    for kk in (32, 65):   # the wider keys through the passes
        s2, r2 = _many_records(kk, 20, 6000, 13 + kk)
        reach2 = GC.reach_of(product, r2)
        _both(product, monkeypatch, lambda: product.Graph.from_seqs(s2, kk, 1, reach=reach2), passes=3)


def test_from_files(product, monkeypatch, tmp_path):
    """the text is made on the device from a FASTA file and a gzip FASTQ file"""
    k = 31
    seqs, records = _many_records(k, 30, 8000, 14)
    fa, fq = tmp_path / "a.fa", tmp_path / "b.fq.gz"
    fa.write_text(">g\n" + seqs[0] + "\n")
    with gzip.open(str(fq), "wt") as f:
        f.write("@r\n%s\n+\n%s\n" % (seqs[1], "I" * len(seqs[1])))
    reach = GC.reach_of(product, records)
    csv = "%s,%s" % (fa, fq)
    info = _both(product, monkeypatch, lambda: product.Graph.from_files(csv, k, 1, reach=reach))
    from_seqs = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach))
    assert info["kept_kmers"] == from_seqs["kept_kmers"] and info["full_kmers"] == from_seqs["full_kmers"]
    assert 0 < info["kept_kmers"] < info["full_kmers"]
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", "2500")
    _both(product, monkeypatch, lambda: product.Graph.from_files(csv, k, 1, reach=reach), passes=3)
    monkeypatch.delenv("G2S_BUILD_PASS_KEYS")
    a = product.Graph.from_files(csv, k, 1, reach=reach, reach_mode=product.REACH_NEVER)
    b = product.Graph.from_files(csv, k, 1)
    try:
        assert not a.bounded
        GC.assert_same_graph(a, b)
    finally:
        a.free()
        b.free()


def test_a_queue_that_has_to_grow(product, monkeypatch):
    k = 31
    seqs, records = _many_records(k, 40, 9000, 12)
    reach = GC.reach_of(product, records)
    want = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach))
    assert want["regrowths"] == 0 and want["kept_kmers"] > 64
    monkeypatch.setenv("G2S_REACH_QUEUE_CAP", "64")
    info = _both(product, monkeypatch, lambda: product.Graph.from_seqs(seqs, k, 1, reach=reach))
    assert info["regrowths"] >= 1 and info["on_device"] == 1   # 64 -> 256 -> ...: the device finished it
    assert info["kept_kmers"] == want["kept_kmers"]


# ---- fills on a bounded graph

FIELDS = ("count", "left_fuz", "right_fuz", "flags", "fill_len", "draws", "phaseC_count", "lengths", "substats", "fill", "backtrace_msg")


def _fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def _fill_workload(product, k, ngaps=50, fuz=10):
    reads = product.G2S.synth_genome(40000, 3, 20240500 + k)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    scaf = product.G2S.synth_gaps(reads, k, fuz, ngaps, 20, 60, 20240600 + k)
    return seqs, scaf, fuz


def _run(product, graph, scaf, k, fuz, d_err, jobs):
    sess = product.Session(graph, 0, d_err=d_err, randseed=SEED)
    try:
        text = sess.execute_scaffolds(scaf, k, solid=1, max_fuz=fuz)
        sess.srand(SEED)
        return text, [_fields(r) for r in sess.fill_batch(jobs)]
    finally:
        sess.destroy()


@pytest.mark.parametrize("resident", ["0", "1"])
@pytest.mark.parametrize("d_err", [50, 300])
@pytest.mark.parametrize("k", [31, 32, 63])
def test_fills_on_the_bounded_graph_equal_fills_on_the_whole_graph(product, monkeypatch, k, d_err, resident):
    """at the sound radius nothing of any fill is lost: FASTA, log, and every record field and fill text of the list"""
    monkeypatch.setenv("G2S_RESIDENT", resident)
    seqs, scaf, fuz = _fill_workload(product, k)
    reach = product.scaffolds_reach(scaf, k, fuz, d_err)
    assert len(reach) >= 45
    # the records' own gaps as a list (their flanks are supersets of the scanner's: the sound radius covers them too)
    jobs = [g for g, _ in reach if g.lmf >= 0 and len(g.right) >= k + g.rmf]
    u = product.Graph.from_seqs(seqs, k, 1, reach=reach)
    info = product.test_last_graph_reach()
    w = product.Graph.from_seqs(seqs, k, 1)
    try:
        assert info["on_device"] == 1 and u.bounded and 0 < u.num_kmers < w.num_kmers
        assert u.validate() == (0, "")
        got, got_list = _run(product, u, scaf, k, fuz, d_err, jobs)
        want, want_list = _run(product, w, scaf, k, fuz, d_err, jobs)
    finally:
        u.free()
        w.free()
    # (a scaffold's N-run is the true length, the closing path k longer: nothing fills while d_err < k — the CPU oracle
    # fills 0 of 50 at k = 63, d_err = 50 and 50 of 50 elsewhere; that case still compares the searches' statistics)
    assert got[2] == want[2] >= 45 and got[3] == want[3]
    assert want[3] > got[2] // 3 if d_err >= k else want[3] == 0
    assert got[0] == want[0] and got[1] == want[1]
    for i, (a, b) in enumerate(zip(got_list, want_list)):
        assert a == b, "gap %d" % i


def test_the_cap(product, monkeypatch):
    """the capability: a read set over the cap fills, with the results of the uncapped whole graph"""
    k, d_err = 31, 50
    seqs, scaf, fuz = _fill_workload(product, k)
    reach = product.scaffolds_reach(scaf, k, fuz, d_err)
    jobs = [g for g, _ in reach if g.lmf >= 0 and len(g.right) >= k + g.rmf]
    w = product.Graph.from_seqs(seqs, k, 1)
    full = w.num_kmers
    want = _run(product, w, scaf, k, fuz, d_err, jobs)
    w.free()
    monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(full - 1))
    with pytest.raises(product.G2SError) as e:
        product.Graph.from_seqs(seqs, k, 1)
    assert TOO_MANY in str(e.value)
    kept = None
    for mode in (product.REACH_ALWAYS, product.REACH_AUTO):
        u = product.Graph.from_seqs(seqs, k, 1, reach=reach, reach_mode=mode)
        try:
            info = product.test_last_graph_reach()
            assert u.bounded and info["on_device"] == 1 and info["full_kmers"] == full and 0 < u.num_kmers < full - 1
            kept = u.num_kmers
            assert _run(product, u, scaf, k, fuz, d_err, jobs) == want
        finally:
            u.free()
    for cap in (kept, kept - 1):   # the cap at or below the kept count: the bounded build is refused the same way
        monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(cap))
        for mode in (product.REACH_ALWAYS, product.REACH_AUTO):
            with pytest.raises(product.G2SError) as e:
                product.Graph.from_seqs(seqs, k, 1, reach=reach, reach_mode=mode)
            assert TOO_MANY in str(e.value)
    monkeypatch.setenv("G2S_BUILD_MAX_KMERS", str(kept + 1))
    product.Graph.from_seqs(seqs, k, 1, reach=reach).free()


# ---- the scanner's jobs lie inside the records' windows (G2S_JOBS_DUMP), on the texts of the host test

def test_every_job_of_the_scanner_lies_inside_its_record(product, monkeypatch, tmp_path):
    import test_graph_reach as H
    d_err = 50
    for name, (k, fuz, text) in sorted(H.scaffold_texts().items()):
        flat = [ln for ln in text.splitlines() if not ln.startswith(">")]
        reads = [s.replace("N", "A").replace("n", "C") for s in flat if s]
        records = product.scaffolds_reach(text, k, fuz, d_err)
        by_run, at = {}, 0
        for ri, seq in enumerate(flat):
            for istart, iend in H._runs(seq):
                by_run[(ri, istart)] = records[at]
                at += 1
        assert at == len(records)
        dump = tmp_path / (name + ".jobs")
        monkeypatch.setenv("G2S_JOBS_DUMP", str(dump))
        g = product.Graph.from_seqs(reads, k, 1)
        sess = product.Session(g, 0, d_err=d_err, randseed=SEED)
        try:
            sess.execute_scaffolds(text, k, solid=1, max_fuz=fuz)
        finally:
            sess.destroy()
            g.free()
            monkeypatch.delenv("G2S_JOBS_DUMP")
        lines = dump.read_text().splitlines() if dump.exists() else []
        assert lines, name
        for ln in lines:
            rec, istart, iend, start, lmf, rmf, gap, left, right = ln.split()
            rec, istart, iend, start, lmf, rmf, gap = (int(x) for x in (rec, istart, iend, start, lmf, rmf, gap))
            want, radius = by_run[(rec, istart)]
            assert want.left.endswith(left) and want.right == right and lmf <= want.lmf and rmf == want.rmf and gap == want.gap_len
            assert radius >= max(0, gap + d_err) + lmf + rmf
            fill = dict(left=left, right=right, gap_len=gap, lmf=lmf, rmf=rmf)
            mine = dict(left=want.left, right=want.right, gap_len=want.gap_len, lmf=want.lmf, rmf=want.rmf)
            assert set(RC.seeds_of(fill, k)) <= set(RC.seeds_of(mine, k))


# ---- the command line

def _core(args, env_extra=None):
    env = dict(os.environ)
    for name in ("G2S_BUILD_REACH", "G2S_BUILD_MAX_KMERS", "G2S_SAVE_GRAPH", "G2S_HOST_BUILD"):
        env.pop(name, None)
    env.update(env_extra or {})
    r = subprocess.run([CORE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_the_command_line(product, tmp_path):
    k, fuz = 8, 11   # -fuz > -k
    reads = product.G2S.synth_genome(20000, 0, 77)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    genome = seqs[0]
    rec = cases.scaffold_record(genome, k, fuz, [(3000, 40, 40), (3000 + 40 + 2 * k + 5, 30, 30)], pad=30)
    (tmp_path / "reads.fa").write_text(reads)
    (tmp_path / "scaf.fa").write_text(">two\n" + rec + "\n>one\n" + cases.scaffold_record(genome, k, fuz, [(9000, 50, 50)], pad=30) + "\n")
    common = ["-reads", str(tmp_path / "reads.fa"), "-k", str(k), "-solid", "1", "-fuz", str(fuz), "-dist-error", "30", "-randseed", "3",
              "-nb-cores", "1"]
    out = {}
    for reach in ("0", "1", "auto"):
        filled = tmp_path / ("filled_%s.fa" % reach)
        r = _core(common + ["-scaffolds", str(tmp_path / "scaf.fa"), "-filled", str(filled), "-reach", reach])
        out[reach] = (filled.read_text(), r.stdout.replace(str(filled), "FILLED"))
    assert out["1"] == out["0"] == out["auto"] and "Filled " in out["0"][1]
    single = {}
    for reach in ("0", "1"):
        filled = tmp_path / ("single_%s.fa" % reach)
        r = _core(common + ["-left", genome[12000 - k - fuz:12000], "-right", genome[12040:12040 + k + fuz], "-length", "40",
                            "-filled", str(filled), "-reach", reach])
        single[reach] = (filled.read_text(), r.stdout.replace(str(filled), "FILLED"))
    assert single["1"] == single["0"]
    cache = tmp_path / "reads.fa.g2s"
    r = _core(common + ["-scaffolds", str(tmp_path / "scaf.fa"), "-filled", str(tmp_path / "f2.fa"), "-reach", "1"], {"G2S_SAVE_GRAPH": "1"})
    assert not cache.exists() and "not saved" in r.stderr
    _core(common + ["-scaffolds", str(tmp_path / "scaf.fa"), "-filled", str(tmp_path / "f3.fa")], {"G2S_SAVE_GRAPH": "1"})
    assert cache.exists()   # (auto under the cap: the whole graph, cached as ever)
