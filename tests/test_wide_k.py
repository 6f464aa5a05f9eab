"""k-mer lengths 64 to 127 on the host: the 256-bit k-mer word (kmer.hpp: u256, KmerOps<u256>), the host graph build
against the string restatement (oracle/pyref.py), the graph cache at 32-byte k-mers and the accepted range of k; and
the CPU oracle's own 256-bit word (oracle/g2s_oracle.cpp: W256) against pyref.
No GPU: without a device the build runs on the host threads."""
import os
import random
import re
import shutil
import subprocess

import pytest

import cases
import pyref
from test_oracle import _compare_with_pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gap2seq_amd", "csrc")
M256 = (1 << 256) - 1


def _reads(k):
    """two reads that share a stretch, with N/n breaks and lower case"""
    rng = cases.SplitMix(1000 + k)
    seqs = [cases.random_dna(rng, 1500) for _ in range(2)]
    seqs[1] = seqs[1][:60] + "N" + seqs[0][40:400] + "n" + seqs[1][420:]
    seqs[0] = seqs[0][:700] + seqs[0][700:900].lower() + seqs[0][900:]
    return seqs


def _check_graph(product, g, p, seqs, k):
    assert g.k == k
    assert g.num_kmers == len(p.kmers)
    for s in seqs:
        for i in range(0, len(s) - k, 7):
            x = pyref.norm(s[i:i + k])
            v = g.node(s[i:i + k])
            if not p.contains(x):
                assert v == product.G2S_INVALID_NODE
                continue
            assert g.node_string(v) == x
            if pyref.revcomp(x) != x:  # the orientation bit is unitig-relative: only v^1 == revcomp is promised
                assert g.node(pyref.revcomp(x)) == v ^ 1
                assert g.node_string(v ^ 1) == pyref.revcomp(x)
            for y in (x, pyref.revcomp(x)):
                w = g.node(y)
                assert [g.node_string(t) for t in g.successors(w)] == p.succ(y)
                assert [g.node_string(t) for t in g.predecessors(w)] == p.pred(y)  # GATB order T,G,A,C


@pytest.mark.parametrize("k", [64, 65, 77, 96, 101, 127])
def test_wide_graph_matches_python_restatement(product, k):
    seqs = _reads(k)
    for solid in (1, 2):
        g = product.Graph.from_seqs(seqs, k, solid, nthreads=3)
        p = pyref.Graph(seqs, k, solid)
        assert len(p.kmers) > (1000 if solid == 1 else 200)
        _check_graph(product, g, p, seqs, k)
        assert g.validate()[0] == 0
        g.free()


@pytest.mark.parametrize("k", [96, 101])
def test_wide_graph_cache_round_trip(product, tmp_path, k):
    seqs = _reads(k)
    g = product.Graph.from_seqs(seqs, k, 1, nthreads=2)
    path = str(tmp_path / ("g%d.g2s" % k))
    g.save(path)
    # header (8 + 32 bytes), then per k-mer: 32-byte k-mer, rank2id, flip, succ, pred (even k), lastnt
    per = 32 + 4 + 1 + 32 + (32 if k % 2 == 0 else 0) + 2
    assert os.path.getsize(path) == 40 + per * g.num_kmers
    h = product.Graph.load(path)
    assert h.num_unitigs == g.num_unitigs
    _check_graph(product, h, pyref.Graph(seqs, k, 1), seqs, k)
    for s in seqs:
        for i in range(0, len(s) - k, 11):
            assert h.node(s[i:i + k]) == g.node(s[i:i + k])
    assert h.validate()[0] == 0
    h.free()
    g.free()


@pytest.mark.parametrize("k", [0, 128])
def test_k_out_of_range_is_rejected(product, k):
    with pytest.raises(product.G2SError, match=r"\[1,127\]"):
        product.Graph.from_seqs(["ACGT" * 100], k, 1)


# ---- the 256-bit word itself, against Python integers ----------------------------------------------------------------

_U256_PROBE = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include "kmer.hpp"
using namespace g2s;
static u256 rd(const char* h) {
  u256 x;
  for (const char* p = h; *p; p++) { int d = *p <= '9' ? *p - '0' : *p - 'a' + 10; x = (x << 4) | (u256)(uint64_t)d; }
  return x;
}
static void pr(const u256& x) {
  printf("%016llx%016llx%016llx%016llx", (unsigned long long)x.word(3), (unsigned long long)x.word(2),
         (unsigned long long)x.word(1), (unsigned long long)x.word(0));
}
int main() {
  char op[16], a[300], b[300];
  int s;
  while (scanf("%15s", op) == 1) {
    if (!strcmp(op, "shl") || !strcmp(op, "shr")) {
      scanf("%299s %d", a, &s);
      pr(op[2] == 'l' ? rd(a) << s : rd(a) >> s);
    } else if (!strcmp(op, "bin")) {
      scanf("%299s %299s", a, b);
      const u256 x = rd(a), y = rd(b);
      pr(x | y); printf(" "); pr(x & y); printf(" "); pr(x ^ y); printf(" "); pr(~x); printf(" "); pr(x - y);
      printf(" %d %d %d", (int)(x == y), (int)(x != y), (int)(x < y));
      printf(" %llu %u %u", (unsigned long long)(uint64_t)x, (unsigned)(uint32_t)x, (unsigned)(uint8_t)x);
    } else if (!strcmp(op, "kmer")) {
      scanf("%299s %d", a, &s);  // a: k characters
      u256 c;
      int strand;
      encode_kmer<u256>(a, s, &c, &strand);
      pr(c); printf(" %d ", strand); pr(KmerOps<u256>::mask(s)); printf(" ");
      pr(KmerOps<u256>::revcomp(c, s));
      printf(" %s %s", decode_kmer<u256>(c, strand, s).c_str(), decode_kmer<u256>(c, 1 - strand, s).c_str());
      KmerRoller<u256> r(s);
      bool full = false;
      for (int i = 0; i < s; i++) full = r.push(a[i]);
      printf(" %d ", (int)full); pr(r.canonical());
    }
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def u256_probe(tmp_path_factory):
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++")
    d = tmp_path_factory.mktemp("u256")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write(_U256_PROBE)
    subprocess.check_call([cxx, "-x", "c++", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


def _hex(x):
    return "%064x" % (x & M256)


def test_u256_shifts_are_exact(u256_probe):
    rnd = random.Random(256)
    vals = [M256, 1, 1 << 255, 0x0123456789abcdef << 100] + [rnd.getrandbits(256) for _ in range(12)]
    shifts = [0, 1, 2, 31, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 254, 255]
    cases_ = [(op, v, s) for op in ("shl", "shr") for v in vals for s in shifts]
    out = u256_probe(["%s %s %d" % (op, _hex(v), s) for op, v, s in cases_])
    for (op, v, s), got in zip(cases_, out):
        want = (v << s) & M256 if op == "shl" else v >> s
        assert got == _hex(want), (op, hex(v), s)


def test_u256_bitwise_compare_and_casts(u256_probe):
    rnd = random.Random(257)
    pairs = [(0, 0), (M256, M256), (1 << 128, (1 << 128) - 1), ((1 << 64) + 5, (1 << 64) + 5), (3, 1 << 200)]
    pairs += [(rnd.getrandbits(256), rnd.getrandbits(256)) for _ in range(20)]
    hi = rnd.getrandbits(128) << 128
    pairs += [(hi | 7, hi | 9), (hi | 9, hi | 7)]  # equal high halves: the low half decides
    out = u256_probe(["bin %s %s" % (_hex(x), _hex(y)) for x, y in pairs])
    for (x, y), got in zip(pairs, out):
        f = got.split()
        assert f[:5] == [_hex(x | y), _hex(x & y), _hex(x ^ y), _hex(~x), _hex(x - y)]
        assert f[5:8] == [str(int(x == y)), str(int(x != y)), str(int(x < y))]
        assert f[8:] == [str(x & (2**64 - 1)), str(x & (2**32 - 1)), str(x & 255)]


def test_u256_kmer_codec(u256_probe):
    rng = cases.SplitMix(77)
    code = {"A": 0, "C": 1, "T": 2, "G": 3}
    items = []
    for k in (1, 31, 32, 63, 64, 65, 96, 127, 128):
        for _ in range(3):
            items.append((k, cases.random_dna(rng, k)))
    items.append((127, "G" * 127))
    items.append((64, "ACGT" * 16))  # a palindrome: strand 1 (the tie rule)
    out = u256_probe(["kmer %s %d" % (s, k) for k, s in items])
    for (k, s), got in zip(items, out):
        f = got.split()
        val = lambda t: int("".join("%d" % code[c] for c in t), 4)  # first base most significant
        fwd, rc = val(s), val(pyref.revcomp(s))
        c, strand = (fwd, 0) if fwd < rc else (rc, 1)
        assert f[0] == _hex(c) and f[1] == str(strand), (k, s)
        assert f[2] == _hex((1 << (2 * k)) - 1)
        assert f[3] == _hex(rc if strand == 0 else fwd)
        assert f[4] == s and f[5] == pyref.revcomp(s)
        assert f[6] == "1" and f[7] == _hex(c)


# ---- the oracle's 256-bit word, against pyref -------------------------------------------------------------------------

@pytest.mark.parametrize("k", [64, 65, 96, 127])
def test_oracle_at_wide_k_equals_python_restatement(oracle, k):
    """the oracle's fill_gap at k >= 64 against pyref in all three fill modes: counts, fuz, draws, Q7 flags, work
    counters, fill text and subgraph statistics.  The fixture puts both strands of a k-mer at one depth (Q7); at even
    k its hairpins hold palindromic k-mers."""
    seqs, gaps = cases.strand_flip_genome(k, 4000, k)
    if k % 2 == 0:
        assert any(seqs[0][i:i + k] == pyref.revcomp(seqs[0][i:i + k]) for i in range(len(seqs[0]) - k + 1))
    e = k + 10
    for skip, allp in ((False, True), (False, False), (True, True)):
        q7 = []
        filled = _compare_with_pyref(oracle, seqs, k, gaps, e, skip, allp, q7)
        assert len(q7) == len(gaps) == 20
        assert filled >= 12 and sum(q7) >= 3, (filled, sum(q7))


@pytest.mark.parametrize("k", [63, 64, 65, 96, 127])
def test_oracle_kmer_counts_at_wide_k(oracle, k):
    """the solid k-mer set: reads with N/n breaks, lower case, a read shorter than k and reads seen two and three times"""
    seqs = _reads(k)
    seqs += [seqs[0][100:900], seqs[0][300:1100], seqs[1][:k - 1], seqs[1][200:200 + k]]
    for solid in (1, 2, 3):
        og = oracle.OracleGraph(seqs, k, solid)
        try:
            assert og.num_kmers == len(pyref.Graph(seqs, k, solid).kmers), solid
        finally:
            og.free()


def test_oracle_rejects_k_above_127(oracle):
    L = oracle.lib()
    arr = (oracle.C.c_char_p * 1)(b"ACGT" * 100)
    assert not L.orc_graph_from_seqs(arr, 1, 128, 1)
    assert not L.orc_graph_from_seqs(arr, 1, 0, 1)
    h = L.orc_graph_from_seqs(arr, 1, 127, 1)
    assert h and L.orc_graph_num_kmers(h) > 0
    L.orc_graph_free(h)


def _gap_lines(log):
    return [ln for ln in log.splitlines() if ln.startswith(("Scaffold:", "SubgraphStats:")) or re.match(r"Filled \d+ gaps out of \d+$", ln)]


def test_oracle_scaffold_mode_at_k127_equals_python_restatement(oracle):
    """execute_scaffolds at k = 127: FASTA and per-gap log lines of the oracle equal pyref's, with a multi-gap record"""
    k, fuz, e = 127, 10, 100
    seqs = cases.toy_genome(k, 12000, k, repeats=10, tandem=2, snp_every=400)
    gl = cases.cut_gaps(k, seqs[0], k, fuz, 16, 50, 400, e)
    records = [("g%d" % i, g["left"] + "N" * g["gap_len"] + g["right"]) for i, g in enumerate(gl)]
    records.append(("multi", cases.scaffold_record(seqs[0], k, fuz, [(1000 + 1500 * j, 60 + 7 * j, 60 + 7 * j + 3) for j in range(6)])))
    text = "".join(">%s\n%s\n" % r for r in records)
    og = oracle.OracleGraph(seqs, k, 1)
    try:
        for skip in (False, True):
            fa, log, sm = oracle.execute_scaffolds(og, text, k, solid=1, d_err=e, max_fuz=fuz, randseed=1, skip_confident=skip)
            pfa, plog, pfilled, pgaps = pyref.execute_scaffolds(pyref.Graph(seqs, k, 1), records, k, e, fuz, 1, skip_confident=skip)
            assert (sm.gaps, sm.filled) == (pgaps, pfilled) == (22, pfilled)
            assert 5 <= pfilled < 22
            assert fa == pfa
            assert _gap_lines(log) == _gap_lines(plog)
    finally:
        og.free()
