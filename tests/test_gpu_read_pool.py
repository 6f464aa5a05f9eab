"""Read pools on the MI355X: the pooled set build on the device (gap2seq_amd/csrc/dbg_gpu.hip: the pool's k-mers
extracted once, the shared list sorted once and merged into every flagged set) against the host build and against the
device set build of the expanded lists; the fills on a pooled graph against the fills on the expanded graph and the
CPU oracle; the filter's pool with the joins on the device; and Gap2Seq-libraries, which uses both, against a
restatement of the wrapper's per-gap flow on libraries where some gaps take the unmapped reads and some do not."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bamwriter as BW  # noqa: E402
import oracle_lib as O  # noqa: E402
import pool_cases as PC  # noqa: E402
import readfilter_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")
SEED = 7


# ---- the device pool build

def _device_pool(product, monkeypatch, capfd, seqs, set_lists, k, solid, shared, set_shared):
    """from_pool on the device; the G2S_DEBUG line must say so"""
    monkeypatch.delenv("G2S_HOST_BUILD", raising=False)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    u = product.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    assert "pooled set graph build" in err and "on the GPU" in err, err[-2000:]
    return u


@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_pool_build_equals_host_pool_build_and_device_set_build(product, monkeypatch, capfd, k, solid):
    for mode in ("shared", "empty", "none"):
        seqs, set_lists, shared, set_shared = PC.pool_workload(k, mode)
        dev = _device_pool(product, monkeypatch, capfd, seqs, set_lists, k, solid, shared, set_shared)
        info = product.test_last_pool_build()
        sets = product.Graph.from_sets(PC.expanded(seqs, set_lists, shared, set_shared), k, solid)  # (device set build)
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
        host = product.Graph.from_pool(seqs, set_lists, k, solid, shared=shared, set_shared=set_shared)
        monkeypatch.delenv("G2S_HOST_BUILD")
        try:
            PC.assert_same_graph(dev, host, len(set_lists))
            PC.assert_same_graph(dev, sets, len(set_lists))
            PC.assert_workload_properties(dev, seqs, k, solid, mode)
            assert info["on_device"] == 1 and info["keys_sorted"] == info["own_positions"] + info["shared_positions"]
            assert product.test_last_pool_build()["on_device"] == 0  # (the host build just made)
        finally:
            dev.free()
            host.free()
            sets.free()


@pytest.mark.parametrize("k", [31, 63, 95])
def test_device_pool_build_on_a_list_of_gaps(product, monkeypatch, capfd, k):
    """the larger workload of the fill tests: overlapping sets, a third of them flagged, sets without own reads"""
    seqs, set_lists, shared, set_shared, _, _ = PC.fill_workload(k, 11 + k, 62)
    dev = _device_pool(product, monkeypatch, capfd, seqs, set_lists, k, 1, shared, set_shared)
    sets = product.Graph.from_sets(PC.expanded(seqs, set_lists, shared, set_shared), k, 1)
    try:
        PC.assert_same_graph(dev, sets, len(set_lists))
    finally:
        dev.free()
        sets.free()


def test_the_shared_list_is_sorted_once(product, monkeypatch, capfd):
    """1, 5 and 40 flagged sets over the same shared list: the keys sorted are the own positions plus the shared
    positions each time"""
    k = 31
    seen = []
    for nflag in (1, 5, 40):
        seqs, set_lists, shared, set_shared, _, _ = PC.fill_workload(k, 19, 46, flag=lambda s, n=nflag: s < n)
        set_shared[-2] = 0  # (the flagged set without own reads: this test counts the flags itself)
        assert sum(set_shared) == nflag and len(set_lists) == 48
        dev = _device_pool(product, monkeypatch, capfd, seqs, set_lists, k, 1, shared, set_shared)
        info = product.test_last_pool_build()
        sets = product.Graph.from_sets(PC.expanded(seqs, set_lists, shared, set_shared), k, 1)
        try:
            own = sum(len(seqs[i]) + 1 for lst in set_lists for i in lst)
            sh = sum(len(seqs[i]) + 1 for i in shared)
            assert info == dict(own_positions=own, shared_positions=sh, keys_sorted=own + sh, on_device=1)
            PC.assert_same_graph(dev, sets, len(set_lists))
            seen.append(info["shared_positions"])
        finally:
            dev.free()
            sets.free()
    assert seen[0] == seen[1] == seen[2] > 10000


# ---- fills on a pooled graph

def _gap(product, g):
    return product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])


def _sequence(g, r):
    if r.count > 0:
        return g["left"][:len(g["left"]) - r.left_fuz] + r.fill
    return g["left"] + "N" * g["gap_len"] + g["right"]


def _oracle_sequence(seqs, g, k):
    if not seqs:
        return g["left"] + "N" * g["gap_len"] + g["right"]
    og = O.OracleGraph(seqs, k, 1)
    try:
        fa, _ = O.execute_single(og, g["left"], g["right"], g["gap_len"], k, solid=1, d_err=PC.D_ERR,
                                 max_fuz=max(g["lmf"], g["rmf"], PC.FUZ), randseed=SEED)
    finally:
        og.free()
    return "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))


def _fields(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.substats, r.phaseC_count, r.lengths)


def _fill(product, graph, gaps, gap_set):
    sess = product.Session(graph, 0, d_err=PC.D_ERR, randseed=SEED)
    try:
        return sess.fill_sets([_gap(product, g) for g in gaps], gap_set)
    finally:
        sess.destroy()


@pytest.mark.parametrize("k,seed,n", [(31, 42, 94), (63, 74, 62), (95, 106, 62)])
def test_fills_on_the_pool_graph_equal_fills_on_the_expanded_graph(product, monkeypatch, capfd, k, seed, n):
    seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, seed, n)
    sets = PC.expanded(seqs, set_lists, shared, set_shared)
    u = _device_pool(product, monkeypatch, capfd, seqs, set_lists, k, 1, shared, set_shared)
    w = product.Graph.from_sets(sets, k, 1)
    try:
        got = _fill(product, u, gaps, gap_set)
        want = _fill(product, w, gaps, gap_set)
    finally:
        u.free()
        w.free()
    filled = flagged_filled = 0
    for i, g in enumerate(gaps):
        assert _fields(got[i]) == _fields(want[i]), "gap %d (set %d)" % (i, gap_set[i])
        assert _sequence(g, got[i]) == _oracle_sequence(sets[gap_set[i]], g, k), "gap %d (set %d)" % (i, gap_set[i])
        filled += got[i].count > 0
        flagged_filled += got[i].count > 0 and set_shared[gap_set[i]] == 1
    assert got[len(gaps) - 1].count == 0 and got[len(gaps) - 1].draws == 0   # the empty set
    assert filled > len(gaps) // 3
    assert flagged_filled > sum(set_shared) // 3                              # fills that came through the shared reads


# ---- the filter's pool with the joins on the device

def test_large_library_pool_device_equals_host(product):
    """the library of test_large_library_device_equals_host (tests/test_gpu_readfilter_gaps.py): the pool from the
    device joins is the pool from the host joins, and its text is the batched filter's"""
    rng = random.Random(31)
    refs, recs, _ = BW.simulate_library(31, n_scaffolds=8, scaffold_len=60000, gap=(30000, 300), pairs=25000,
                                        unmapped_pairs=200, ambiguous=0.01)
    recs = list(recs)
    rng.shuffle(recs)
    bam = BW.bam_bytes(refs, recs)
    scafs = [r[0] for r in refs]
    gaps = []
    for i in range(2000):
        gaps.append((rng.choice(scafs + ["nosuch"] if i % 97 == 0 else scafs), rng.randrange(0, 60000),
                     rng.choice([-1, 0, rng.randrange(1, 500)]), rng.choice([-1, 0, rng.randrange(1, 200)])))
    dev = product.filter_reads_gaps_pool(bam, 300, 20, gaps, device=0)
    host = product.filter_reads_gaps_pool(bam, 300, 20, gaps, device=-1)
    text, _, un = product.filter_reads_gaps(bam, 300, 20, gaps, device=-1, unmapped=True)
    try:
        assert dev.stats["on_device"] == 1 and host.stats["on_device"] == 0 and dev.stats["file_passes"] == 2
        assert dev.total == host.total and dev.n_reads == host.n_reads and dev.nbytes == host.nbytes
        assert dev.seqs == host.seqs and dev.names == host.names and list(dev.unmapped) == list(host.unmapped)
        for i in range(len(gaps)):
            assert dev.gap_reads(i) == host.gap_reads(i), gaps[i]
        assert sum(len(dev.gap_reads(i)) for i in range(len(gaps))) > 10000
        for i in range(0, 2000, 50):
            assert dev.fasta(i) == text[i][0], gaps[i]
        assert dev.unmapped_fasta() == un[0]
    finally:
        dev.free()
        host.free()


# ---- Gap2Seq-libraries on pools: the wrapper's per-gap flow restated (tests/test_gpu_readfilter_gaps.py: _restatement)

K, FUZ, SOLID, DERR, LSEED = 31, 10, 1, 100, 3
GENOME = 6000
LIBRARY_GAP = (3000, 500)   # missing from the scaffold; longer than the inserts: its middle is in unmapped pairs only
# pairs, mean, sd, threshold.  The thresholds add up to 135 filtered bases a gap base: the restatement puts the 16 gaps
# below at 12.2 (the long one), 98.7 to 128.5 (seven) and 142.8 to 302.6 (eight), so eight gaps take the unmapped reads
# and eight do not.
LIBRARIES = [(1500, 300, 20, 45.0), (800, 250, 30, 45.0), (1000, 350, 0, 45.0)]
# (bp, gap length, N or n, bases of the genome between the flanks beyond the gap's length)
GAPS = [(3000, 500, "N", 0), (700, 100, "N", 0), (2200, 150, "n", 0), (1000, 40, "N", 0), (4600, 80, "N", 0),
        (5200, 120, "N", 0), (3900, 60, "n", 0), (1600, 90, "N", 0), (450, 60, "N", 400), (5600, 30, "N", 0),
        (2600, 70, "N", 0), (4200, 50, "N", 250), (1300, 200, "N", 0), (1900, 180, "N", 0), (4900, 160, "N", 0),
        (5400, 140, "N", 0)]


def libraries_case():
    """(libs, records, bed): libs = [(bam bytes, mean, sd, threshold)]"""
    libs = []
    for i, (pairs, mean, sd, thr) in enumerate(LIBRARIES):
        refs, recs, _ = BW.simulate_library(23, n_scaffolds=1, scaffold_len=GENOME, gap=LIBRARY_GAP, pairs=pairs, mean=mean,
                                            sd=sd, unmapped_pairs=150, ambiguous=0.0)
        libs.append((BW.bam_bytes(refs, recs, block=[65280, 5000, 700][i]), mean, sd, thr))
    rng = random.Random(23)
    genome = "".join(rng.choice("ACGT") for _ in range(GENOME))  # (simulate_library's first draws)
    fl = K + FUZ
    records, bed = [], []
    for j, (bp, gl, ch, extra) in enumerate(GAPS):
        seq = genome[bp - fl:bp] + ch * gl + genome[bp + gl + extra:bp + gl + extra + fl]
        records.append(">scaf0 scaffold 0 contig %d gap %d\n%s\n" % (j, j, seq))
        bed.append("scaf0\t%d\t%d\n" % (bp - fl, bp + gl + extra + fl))
    return libs, records, bed


def _seqs(fasta):
    out, cur = [], None
    for ln in fasta.splitlines():
        if ln.startswith(">"):
            if cur is not None:
                out.append(cur)
            cur = ""
        elif cur is not None:
            cur += ln
    if cur is not None:
        out.append(cur)
    return out


def _grep_bytes(fasta):
    """grep '^[^>;]' | wc -c (Gap2Seq.py:156-159)"""
    return sum(len(ln) for ln in fasta.splitlines(keepends=True) if ln and ln[0] not in ">;\n")


def _parse_gap(record, bed_line):
    """Gap2Seq.py:246-262"""
    lines = record.split("\n")
    comment, gap = lines[0], "".join(lines[1:])
    left = gap[:gap.upper().find("N")]
    right = gap[gap.upper().rfind("N") + 1:]
    cols = bed_line.rstrip().split("\t")
    return dict(comment=comment, left=left, right=right, flank=min(len(left), len(right)),
                gap=len(gap) - len(left) - len(right), scaffold=cols[0], bp=int(cols[1]) + len(left))


def restatement(libs, records, bed_lines, fill=True):
    """(output text, last line, per gap: whether it took the unmapped reads, per gap: filtered bases a gap base)"""
    unmapped = [REF.read_filter(data, mean, sd, "0", 0, gap_length=0, unmapped_only=True)[0] for data, mean, sd, _ in libs]
    threshold = sum(t for _, _, _, t in libs)
    out, ok, took, ratios = "", 0, [], []
    for rec, bl in zip(records, bed_lines):
        g = _parse_gap(rec, bl)
        reads, flen = [], 0
        for data, mean, sd, _ in libs:
            fa = REF.read_filter(data, mean, sd, g["scaffold"], g["bp"], gap_length=g["gap"], flank_length=g["flank"])[0]
            reads += _seqs(fa)
            flen += _grep_bytes(fa)
        ratios.append(flen / g["gap"])
        took.append(flen / g["gap"] < threshold)
        if took[-1]:
            for fa in unmapped:
                reads += _seqs(fa)
        text = g["left"] + "N" * g["gap"] + g["right"]
        if reads and fill:
            og = O.OracleGraph(reads, K, SOLID)
            try:
                fa, _ = O.execute_single(og, g["left"], g["right"], g["gap"], K, solid=SOLID, d_err=DERR, max_fuz=FUZ,
                                         randseed=LSEED)
            finally:
                og.free()
            text = "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))
        ok += "N" not in text and "n" not in text
        out += g["comment"] + "\n" + text + "\n"
    return out, "Filled %i out of %i gaps" % (ok, len(records)), took, ratios


@pytest.mark.parametrize("filter_device", [None, "-1"])
def test_libraries_on_pools_match_the_wrapper_flow(product, tmp_path, filter_device):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    libs, records, bed = libraries_case()
    for i, (data, _, _, _) in enumerate(libs):
        (tmp_path / ("lib%d.bam" % i)).write_bytes(data)
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), m, s, t)
                                               for i, (_, m, s, t) in enumerate(libs)))
    want_text, want_line, took, _ = restatement(libs, [r.rstrip("\n") for r in records], bed)
    # both kinds of gap, by the restatement itself: a quarter of the gaps at least on each side of the threshold
    assert sum(took) >= (len(GAPS) + 3) // 4 and len(took) - sum(took) >= (len(GAPS) + 3) // 4, took
    assert took[0]  # the gap longer than the inserts: its middle comes from the unmapped reads alone
    argv = [EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
            str(tmp_path / "gaps.bed"), "-filled", str(tmp_path / "out.fa"), "-k", str(K), "-fuz", str(FUZ),
            "-solid", str(SOLID), "-dist-error", str(DERR), "-randseed", str(LSEED)]
    if filter_device is not None:
        argv += ["-filter-device", filter_device]
    run = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert (tmp_path / "out.fa").read_text() == want_text
    assert run.stdout.strip().splitlines()[-1] == want_line
    assert int(want_line.split()[1]) >= len(GAPS) - 4
