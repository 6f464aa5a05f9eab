"""The solid k-mer set of a single graph counted in key-range passes on the device (gap2seq_amd/csrc/solid_passes.h):
histogram of the keys, passes planned on the host, one extract + sort + run-length pass per key range.  The pass form is
forced with G2S_BUILD_PASS_KEYS (the keys a pass may hold) on read sets the one-sort count takes as well, and its graph
must be the one-sort graph word for word — the solid set is the same sorted array — and the host build's by k-mer strings.
g2s_test_last_solid_count keeps a case from passing through a fallback."""
import random

import pytest

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF


def _reads(k):
    """the read set of test_gpu_graph_build_solid_threshold_and_wide_kmers"""
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


def _valid_keys(reads, k):
    n = 0
    for r in reads:
        bad = -1  # the last invalid character
        for i, c in enumerate(r):
            if c in "Nn":
                bad = i
            if i >= k - 1 and i - bad >= k:
                n += 1
    return n


def _build(product, monkeypatch, reads, k, solid, mode, cap=None, piece=None):
    for name in ("G2S_HOST_BUILD", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES"):
        monkeypatch.delenv(name, raising=False)
    if mode == "host":
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
    if mode == "pass":
        monkeypatch.setenv("G2S_BUILD_PASS_KEYS", str(cap))
        if piece is not None:
            monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", str(piece))
    g = product.Graph.from_seqs(reads, k, solid)
    info = product.test_last_solid_count()
    for name in ("G2S_HOST_BUILD", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES"):
        monkeypatch.delenv(name, raising=False)
    return g, info


@pytest.fixture(scope="module")
def refs():
    """the one-sort device graph and the host graph of a read set, built once: {key: (one-sort, host)}"""
    cache = {}
    yield cache
    for pair in cache.values():
        for g in pair:
            g.free()


def _refs(refs, product, monkeypatch, key, reads, k, solid):
    if key not in refs:
        one, info = _build(product, monkeypatch, reads, k, solid, "sort")
        assert (info["on_device"], info["passes"]) == (1, 0)
        host, info = _build(product, monkeypatch, reads, k, solid, "host")
        assert (info["on_device"], info["passes"]) == (0, 0)
        refs[key] = (one, host)
    return refs[key]


def _assert_equal_graphs(product, gp, one, host, k, sample_from, seed):
    assert gp.num_kmers == one.num_kmers
    a, b = product.test_graph_tables(gp), product.test_graph_tables(one)
    assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])  # same sorted set: the same node ids
    assert (gp.num_kmers, gp.num_unitigs) == (host.num_kmers, host.num_unitigs)
    assert gp.validate() == (0, "") and host.validate() == (0, "")
    rr = random.Random(seed)
    for _ in range(300):
        s = rr.choice(sample_from)
        if len(s) < k:
            continue
        p = rr.randrange(0, len(s) - k + 1)
        km = s[p:p + k].upper()
        x, y = gp.node(km), host.node(km)
        assert (x == INVALID) == (y == INVALID)
        if x != INVALID:
            assert gp.node_string(x) == km and host.node_string(y) == km
            assert [gp.node_string(v) for v in gp.successors(x)] == [host.node_string(v) for v in host.successors(y)]
            assert [gp.node_string(v) for v in gp.predecessors(x)] == [host.node_string(v) for v in host.predecessors(y)]


def _pass_case(refs, product, monkeypatch, key, reads, k, solid, cap, sample_from, piece=None, min_passes=2):
    one, host = _refs(refs, product, monkeypatch, key, reads, k, solid)
    gp, info = _build(product, monkeypatch, reads, k, solid, "pass", cap, piece)
    try:
        print("k=%d solid=%d cap=%d piece=%s: %r" % (k, solid, cap, piece, info))
        assert info["on_device"] == 1 and info["passes"] >= min_passes and info["max_pass_keys"] <= cap
        assert info["positions"] == sum(len(r) + 1 for r in reads) and info["solid"] == gp.num_kmers
        _assert_equal_graphs(product, gp, one, host, k, sample_from, k * 7 + solid)
    finally:
        gp.free()
    return info


@pytest.mark.parametrize("cap_kind", ["third", "4096"])
@pytest.mark.parametrize("solid", [1, 2])
@pytest.mark.parametrize("k", [15, 31, 32, 63, 64])
def test_pass_graph_equals_one_sort_and_host(refs, product, monkeypatch, k, solid, cap_kind):
    genome, reads = _reads(k)
    cap = _valid_keys(reads, k) // 3 if cap_kind == "third" else 4096
    info = _pass_case(refs, product, monkeypatch, ("reads", k, solid), reads, k, solid, cap, [genome])
    if cap_kind == "third":
        assert info["passes"] >= 3


@pytest.mark.parametrize("k", [15, 31, 32, 63, 64])
def test_one_forced_pass(refs, product, monkeypatch, k):
    genome, reads = _reads(k)
    valid = _valid_keys(reads, k)
    for cap in (valid, 1 << 24):
        info = _pass_case(refs, product, monkeypatch, ("reads", k, 2), reads, k, 2, cap, [genome], min_passes=1)
        assert info["passes"] == 1 and info["max_pass_keys"] == valid and info["refined_bins"] == 0


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_boundary_keys_every_7mer_twice(refs, product, monkeypatch):
    """Every canonical 7-mer occurs exactly twice, once on each strand and in two reads; with solid 2 a key counted in
    two passes is harmless but one counted in none — or split between two — is lost: all 8 192 must be there."""
    k = 7
    reads = []
    for x in range(4 ** k):
        s = "".join("ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))
        if s < _revcomp(s):  # one of each pair; k is odd, so no k-mer is its own reverse complement
            reads += [s, _revcomp(s)]
    assert len(reads) == 2 * 8192
    random.Random(1).shuffle(reads)
    info = _pass_case(refs, product, monkeypatch, "all7", reads, k, 2, 64, reads)
    assert info["solid"] == 8192 and info["passes"] >= 2 * 8192 // 64
    # and with solid 3 nothing is solid: no pass sees a key three times
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", "64")
    g = product.Graph.from_seqs(reads, k, 3)
    monkeypatch.delenv("G2S_BUILD_PASS_KEYS")
    try:
        assert g.num_kmers == 0 and product.test_last_solid_count()["on_device"] == 1
    finally:
        g.free()


def _skewed_reads(k):
    genome, reads = _reads(k)
    rr = random.Random(99)
    poly_a = ["A" * 400] * 100
    ac = ["AC" * 200] * 100
    # k-mers that share poly-A's leading bases without being it: the bin holds more than poly-A's own count
    near = ["A" * 40 + "".join(rr.choice("ACGT") for _ in range(360)) for _ in range(10)]
    reads = reads + poly_a + ac + near
    count = sum(1 for r in poly_a + near for i in range(len(r) - k + 1) if r[i:i + k] == "A" * k)  # (no poly-T anywhere)
    assert count > 100 * (400 - k + 1) and not any("T" * k in r.upper() for r in reads)
    return genome, reads, near, count


def test_skewed_bin_is_refined(refs, product, monkeypatch):
    """half the text an (AC)n and a poly-A repeat; cap = the occurrences of poly-A's one k-mer, so its bin is beyond cap
    but no single k-mer is"""
    k = 31
    genome, reads, near, poly_a_count = _skewed_reads(k)
    info = _pass_case(refs, product, monkeypatch, "skew", reads, k, 2, poly_a_count, [genome, "A" * 400, "AC" * 200] + near)
    assert info["refined_bins"] >= 1


def test_single_kmer_beyond_cap_takes_the_host_count(refs, product, monkeypatch, capfd):
    k = 31
    genome, reads, near, poly_a_count = _skewed_reads(k)
    one, host = _refs(refs, product, monkeypatch, "skew", reads, k, 2)
    monkeypatch.setenv("G2S_DEBUG", "1")
    capfd.readouterr()
    gp, info = _build(product, monkeypatch, reads, k, 2, "pass", poly_a_count - 1)
    err = capfd.readouterr().err
    monkeypatch.delenv("G2S_DEBUG")
    try:
        assert info["on_device"] == 0 and info["passes"] == 0
        assert "k-mer set on the host (one k-mer occurs %d times" % poly_a_count in err
        _assert_equal_graphs(product, gp, one, host, k, [genome, "A" * 400, "AC" * 200] + near, 5)
    finally:
        gp.free()


@pytest.mark.parametrize("piece", ["100", "1000", "separator", "larger"])
def test_staging_piece_sizes(refs, product, monkeypatch, piece):
    k = 31
    genome, reads = _reads(k)
    assert all(len(r) == 400 for r in reads[:-1])
    text = sum(len(r) + 1 for r in reads)
    # (100: smaller than every read; 1000: pieces end inside reads; 5 reads and their separators; the text in one piece)
    nbytes = {"100": 100, "1000": 1000, "separator": 5 * 401, "larger": text + 4096}[piece]
    cap = _valid_keys(reads, k) // 3
    _pass_case(refs, product, monkeypatch, ("reads", k, 2), reads, k, 2, cap, [genome], piece=nbytes)
