// gap2seq_amd/csrc/dbg.cpp — see dbg.hpp.
#include "dbg.hpp"
#include "reads_text.h"

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <unordered_set>

namespace g2s {

// numbers what the device's list ranking leaves unnumbered (circular unitigs): rank-space successors, the first free id
using HostWalk = std::function<void(const std::vector<uint32_t>&, uint32_t)>;
// dbg_gpu.hip
bool count_solid_gpu(Graph& g, const BuildInput& in, int solid, int device, std::string* why, SolidCountInfo* info);
bool graph_finish_gpu(Graph& g, int device, const HostWalk& host_walk, std::string* why);
bool graph_build_sets_gpu(Graph& g, const std::vector<std::pair<const char*, uint64_t>>& seqs, const std::vector<uint32_t>& seq_set,
                          uint32_t nsets, int solid, int device, const HostWalk& host_walk, std::string* why);
bool graph_build_pool_gpu(Graph& g, const PoolSets& ps, int solid, int device, const HostWalk& host_walk, PoolBuildInfo* info,
                          std::string* why, const PoolReach* reach = nullptr, PoolReachInfo* rinfo = nullptr,
                          bool* device_usable = nullptr);

namespace {

LastInfo<SolidCountInfo> g_solid_info;
LastInfo<GraphReachInfo> g_graph_reach_info;
LastInfo<PoolBuildInfo> g_pool_info;
LastInfo<PoolReachInfo> g_reach_info;

template <class F>
void parallel_for(uint64_t n, int nthreads, F f) {
  if (nthreads <= 1 || n < 4096) { f((uint64_t)0, n, 0); return; }
  std::vector<std::thread> th;
  uint64_t chunk = (n + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; t++) {
    uint64_t b = std::min(n, chunk * t), e = std::min(n, chunk * (t + 1));
    if (b >= e) break;
    th.emplace_back([=]() { f(b, e, t); });
  }
  for (auto& x : th) x.join();
}

// sorted rank of a canonical k-mer, or -1
template <class KT>
int64_t rank_of(const Graph& g, KT x) {
  const std::vector<KT>& v = kmer_vec<KT>(g);
  const int shift = 2 * g.k - g.bucket_bits;
  size_t b = (size_t)(x >> shift);
  size_t lo = g.bucket[b], hi = g.bucket[b + 1];
  while (lo < hi) {
    size_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < g.bucket[b + 1] && v[lo] == x) ? (int64_t)lo : -1;
}

// sorted rank of a canonical k-mer within ranks [lo, hi), or -1 (a set of a set graph)
template <class KT>
int64_t rank_in(const Graph& g, uint64_t lo, uint64_t hi, KT x) {
  const std::vector<KT>& v = kmer_vec<KT>(g);
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (v[(size_t)mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < end && v[(size_t)lo] == x) ? (int64_t)lo : -1;
}

template <class KT>
void build_bucket_index(Graph& g, int max_bits = 22) {
  const std::vector<KT>& v = kmer_vec<KT>(g);
  g.bucket_bits = std::min(2 * g.k, max_bits);
  const int shift = 2 * g.k - g.bucket_bits;
  const size_t nb = (size_t)1 << g.bucket_bits;
  g.bucket.assign(nb + 1, 0);
  for (size_t i = 0; i < v.size(); i++) g.bucket[(size_t)(v[i] >> shift) + 1]++;
  for (size_t b = 0; b < nb; b++) g.bucket[b + 1] += g.bucket[b];
}

// 1. collect canonical k-mers, 2. sort, 3. keep those seen >= solid times
template <class KT>
void count_solid(Graph& g, const std::vector<std::pair<const char*, uint64_t>>& seqs, int solid, int nthreads) {
  const int k = g.k;
  // chunk long sequences so that threads share one chromosome
  struct Chunk { const char* p; uint64_t len; };
  std::vector<Chunk> chunks;
  const uint64_t kChunk = 1 << 20;
  for (auto& s : seqs) {
    if (s.second < (uint64_t)k) continue;
    for (uint64_t off = 0; off + k <= s.second; off += kChunk) {
      uint64_t len = std::min<uint64_t>(kChunk + k - 1, s.second - off);
      chunks.push_back({s.first + off, len});
    }
  }
  nthreads = std::max(1, nthreads);
  std::vector<std::vector<KT>> local((size_t)nthreads);
  std::atomic<size_t> next(0);
  auto work = [&](int t) {
    std::vector<KT>& out = local[(size_t)t];
    while (true) {
      size_t ci = next.fetch_add(1);
      if (ci >= chunks.size()) break;
      KmerRoller<KT> r(k);
      const char* p = chunks[ci].p;
      for (uint64_t i = 0; i < chunks[ci].len; i++)
        if (r.push(p[i])) out.push_back(r.canonical());
    }
  };
  {
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
  }
  // range partition by the top byte so that partitions sort independently
  const int pshift = std::max(0, 2 * k - 8);
  const size_t P = (size_t)1 << std::min(8, 2 * k);
  std::vector<uint64_t> cnt(P + 1, 0);
  for (auto& v : local) for (KT x : v) cnt[(size_t)(x >> pshift) + 1]++;
  for (size_t b = 0; b < P; b++) cnt[b + 1] += cnt[b];
  std::vector<KT> all((size_t)cnt[P]);
  {
    std::vector<uint64_t> pos(cnt.begin(), cnt.end() - 1);
    for (auto& v : local) {
      for (KT x : v) all[(size_t)pos[(size_t)(x >> pshift)]++] = x;
      std::vector<KT>().swap(v);
    }
  }
  {
    std::atomic<size_t> nb(0);
    auto sorter = [&]() {
      while (true) {
        size_t b = nb.fetch_add(1);
        if (b >= P) break;
        std::sort(all.begin() + (ptrdiff_t)cnt[b], all.begin() + (ptrdiff_t)cnt[b + 1]);
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; t++) th.emplace_back(sorter);
    sorter();
    for (auto& x : th) x.join();
  }
  std::vector<KT>& keep = kmer_vec<KT>(g);
  keep.clear();
  for (size_t i = 0; i < all.size();) {
    size_t j = i + 1;
    while (j < all.size() && all[j] == all[i]) j++;
    if ((int64_t)(j - i) >= (int64_t)solid) keep.push_back(all[i]);
    i = j;
  }
  keep.shrink_to_fit();
  g.n = keep.size();
}

// successor / predecessor tables in sorted-rank space
template <class KT>
void build_tables_rank(const Graph& g, int nthreads, std::vector<uint32_t>* succ, std::vector<uint32_t>* pred) {
  const std::vector<KT>& v = kmer_vec<KT>(g);
  const int k = g.k;
  const KT mask = KmerOps<KT>::mask(k);
  const bool even = (k % 2) == 0;
  succ->assign((size_t)g.n * 8, kInvalidNode);
  if (even) pred->assign((size_t)g.n * 8, kInvalidNode);
  parallel_for(g.n, nthreads, [&](uint64_t b, uint64_t e, int) {
    for (uint64_t i = b; i < e; i++) {
      const KT c = v[(size_t)i], rc = KmerOps<KT>::revcomp(c, k);
      for (int strand = 0; strand < 2; strand++) {
        if (strand == 0 && c == rc) continue;  // palindrome: only strand 1 exists (tie rule)
        const KT seq = strand == 0 ? c : rc;
        const KT rseq = strand == 0 ? rc : c;
        const size_t base = ((size_t)i * 2 + strand) * 4;
        for (int nt = 0; nt < 4; nt++) {
          KT y = ((seq << 2) | (KT)nt) & mask;
          KT ry = (rseq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));
          KT cy = y < ry ? y : ry;
          int64_t r = rank_of<KT>(g, cy);
          if (r >= 0) (*succ)[base + nt] = (uint32_t)(2 * r + (y < ry ? 0 : 1));
          if (even) {
            KT z = ((rseq << 2) | (KT)nt) & mask;                 // revcomp of the predecessor
            KT p = (seq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));  // the predecessor
            KT cp = p < z ? p : z;
            int64_t rp = rank_of<KT>(g, cp);
            if (rp >= 0) (*pred)[base + nt] = (uint32_t)(2 * rp + (p < z ? 0 : 1));
          }
        }
      }
    }
  });
}

inline int out_degree(const std::vector<uint32_t>& succ, uint32_t v, uint32_t* only) {
  int d = 0;
  for (int nt = 0; nt < 4; nt++) {
    uint32_t w = succ[(size_t)v * 4 + nt];
    if (w != kInvalidNode) { d++; *only = w; }
  }
  return d;
}

// New node indices in unitig order: k-mers of one maximal non-branching path are
// consecutive, in path order.  rank-space tables in, permutation out.
// With `resume` the k-mers already numbered (by unitig_order_gpu) are kept and the walk
// numbers the rest from first_id on.
void unitig_order(const std::vector<uint32_t>& succ, uint64_t n, bool even_k, std::vector<uint32_t>* rank2id,
                  std::vector<uint8_t>* flip, uint64_t* n_unitigs, bool resume = false, uint32_t first_id = 0) {
  if (!resume) {
    rank2id->assign((size_t)n, kInvalidNode);
    flip->assign((size_t)n, 0);
  }
  uint32_t next_id = resume ? first_id : 0;
  uint64_t unitigs = resume ? *n_unitigs : 0;
  // the unique continuation v -> w when the edge is unitig-internal
  auto step = [&](uint32_t v) -> uint32_t {
    uint32_t w = kInvalidNode, back = kInvalidNode;
    if (out_degree(succ, v, &w) != 1) return kInvalidNode;
    if ((w >> 1) == (v >> 1)) return kInvalidNode;              // self loop / hairpin
    if (out_degree(succ, w ^ 1u, &back) != 1) return kInvalidNode;  // in-degree of w
    if (back != (v ^ 1u)) return kInvalidNode;                  // (palindromes, even k)
    return w;
  };
  for (uint64_t r = 0; r < n; r++) {
    if ((*rank2id)[(size_t)r] != kInvalidNode) continue;
    uint32_t start = (uint32_t)(2 * r);
    if (even_k) {
      // palindromic k-mers have only strand 1; their strand-0 row is empty and isolated
      bool empty0 = true;
      for (int nt = 0; nt < 4; nt++) if (succ[(size_t)start * 4 + nt] != kInvalidNode) empty0 = false;
      uint32_t dummy;
      if (empty0 && out_degree(succ, start | 1u, &dummy) > 0) start |= 1u;
    }
    // walk backwards (= forwards on the reverse strand) to the unitig start
    uint32_t v = start ^ 1u;
    while (true) {
      uint32_t w = step(v);
      if (w == kInvalidNode || (w >> 1) == (start >> 1) || (*rank2id)[w >> 1] != kInvalidNode) break;
      v = w;
    }
    v ^= 1u;  // first node of the unitig, forward orientation
    unitigs++;
    while (true) {
      (*rank2id)[v >> 1] = next_id++;
      (*flip)[v >> 1] = (uint8_t)(v & 1u);  // GATB strand of the numbering direction
      uint32_t w = step(v);
      if (w == kInvalidNode || (*rank2id)[w >> 1] != kInvalidNode) break;
      v = w;
    }
  }
  *n_unitigs = unitigs;
}

// unitig-start bitmap from the id-space successor table (same predicate as unitig_order's step)
void build_ustart(Graph& g) {
  const uint64_t n = g.n;
  g.ustart.assign((size_t)((n + 63) / 64 + 1), 0);
  auto only_out = [&](uint32_t v, uint32_t* w) -> int {
    int c = 0;
    for (int nt = 0; nt < 4; nt++) {
      const uint32_t x = g.succ[(size_t)v * 4 + nt];
      if (x != kInvalidNode) { c++; *w = x; }
    }
    return c;
  };
  for (uint64_t i = 0; i < n; i++) {
    bool internal = false;
    if (i > 0) {
      const uint32_t v = (uint32_t)(2 * (i - 1)), want = (uint32_t)(2 * i);
      uint32_t w = kInvalidNode, back = kInvalidNode;
      internal = only_out(v, &w) == 1 && w == want && only_out(want ^ 1u, &back) == 1 && back == (v ^ 1u);
    }
    if (!internal) g.ustart[(size_t)(i >> 6)] |= 1ull << (i & 63);
  }
  for (uint64_t i = n; i < (uint64_t)g.ustart.size() * 64; i++) g.ustart[(size_t)(i >> 6)] |= 1ull << (i & 63);
}

// ---- the device-first route every builder takes: the device build (dbg_gpu.hip), the host build behind it ----------
Graph* new_graph(int k, int solid) {
  Graph* g = new Graph();
  g->k = k;
  g->solid = solid;
  g->kmer_bytes = kmer_width(k);
  return g;
}

// G2S_HOST_BUILD (set to anything): no builder tries the device.  Read on every call: it changes within a process.
bool host_build_asked() { return getenv("G2S_HOST_BUILD") != nullptr; }

// what the device builds hand the circular unitigs to: unitig_order resuming on g's own numbering
HostWalk host_walk_of(Graph& g) {
  return [&g](const std::vector<uint32_t>& succ_r, uint32_t first_id) {
    unitig_order(succ_r, g.n, (g.k % 2) == 0, &g.rank2id, &g.flip, &g.n_unitigs, true, first_id);
  };
}

// A set builder's device attempt: attempt(g, device, host_walk, &why) on a new graph.  The graph when that succeeds (the
// success line is the caller's: it differs between builders); nullptr for the host build to follow — at once under
// G2S_HOST_BUILD, else after the line "<what> on the host (<why>)".
template <class Attempt>
Graph* build_on_device(int k, int solid, const char* what, Attempt&& attempt) {
  if (host_build_asked()) return nullptr;
  Graph* g = new_graph(k, solid);
  std::string why;
  if (attempt(*g, build_device(), host_walk_of(*g), &why)) return g;
  if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s]   %s on the host (%s)\n", what, why.c_str());
  delete g;
  return nullptr;
}

template <class KT>
void finish_graph_host(Graph& g, int nthreads);

template <class KT>
void finish_graph(Graph& g, int nthreads) {
  const auto f0 = std::chrono::steady_clock::now();
  if (g.bucket.empty()) build_bucket_index<KT>(g);  // (the GPU k-mer set brings its index along)
  // With a GPU: successor table (at even k the predecessor table too) by binary search, numbering
  // along unitigs by list ranking, tables in id space and the unitig-start bitmap all on the device
  // (dbg_gpu.hip); the host only numbers circular unitigs.  Otherwise the host build below, which
  // is the authority on palindromic k-mers (even k) the device build is tested against.
  if (!host_build_asked()) {
    std::string why;
    const bool ok = graph_finish_gpu(g, build_device(), host_walk_of(g), &why);
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s]   tables, unitig order, id space: %.3f s on the %s%s%s\n",
              std::chrono::duration<double>(std::chrono::steady_clock::now() - f0).count(), ok ? "GPU" : "host next (",
              ok ? "" : why.c_str(), ok ? "" : ")");
    if (ok) return;
  }
  finish_graph_host<KT>(g, nthreads);
}

template <class KT>
void finish_graph_host(Graph& g, int nthreads) {
  const auto f0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> succ_r, pred_r;
  build_tables_rank<KT>(g, nthreads, &succ_r, &pred_r);
  const auto f1 = std::chrono::steady_clock::now();
  unitig_order(succ_r, g.n, (g.k % 2) == 0, &g.rank2id, &g.flip, &g.n_unitigs);
  if (getenv("G2S_DEBUG"))
    fprintf(stderr, "[g2s]   index + successor table %.3f s, unitig order %.3f s (host walk)\n",
            std::chrono::duration<double>(f1 - f0).count(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - f1).count());
  g.id2rank.assign((size_t)g.n, 0);
  for (uint64_t r = 0; r < g.n; r++) g.id2rank[g.rank2id[(size_t)r]] = (uint32_t)r;
  // permute tables into id space
  const std::vector<KT>& v = kmer_vec<KT>(g);
  g.succ.assign((size_t)g.n * 8, kInvalidNode);
  if (!pred_r.empty()) g.pred.assign((size_t)g.n * 8, kInvalidNode);
  g.lastnt.assign((size_t)g.n * 2, 0);
  const int k = g.k;
  parallel_for(g.n, nthreads, [&](uint64_t b, uint64_t e, int) {
    auto remap = [&](uint32_t w) -> uint32_t {  // rank-space (GATB strand) -> id-space (unitig orientation)
      return 2 * g.rank2id[w >> 1] + ((w & 1u) ^ (uint32_t)g.flip[w >> 1]);
    };
    for (uint64_t r = b; r < e; r++) {
      const uint32_t id = g.rank2id[(size_t)r];
      for (int s = 0; s < 2; s++) {
        const size_t row = ((size_t)id * 2 + (size_t)(s ^ g.flip[(size_t)r])) * 4;
        for (int nt = 0; nt < 4; nt++) {
          uint32_t w = succ_r[((size_t)r * 2 + s) * 4 + nt];
          if (w != kInvalidNode) g.succ[row + nt] = remap(w);
          if (!pred_r.empty()) {
            uint32_t p = pred_r[((size_t)r * 2 + s) * 4 + nt];
            if (p != kInvalidNode) g.pred[row + nt] = remap(p);
          }
        }
      }
      const KT c = v[(size_t)r];
      const uint8_t last_fwd = (uint8_t)(c & 3), last_rev = (uint8_t)(((c >> (2 * (k - 1))) & 3) ^ 2);
      g.lastnt[(size_t)id * 2 + (size_t)(0 ^ g.flip[(size_t)r])] = last_fwd;
      g.lastnt[(size_t)id * 2 + (size_t)(1 ^ g.flip[(size_t)r])] = last_rev;
    }
  });
  build_ustart(g);
}

// the oriented node of the k characters at s, or kInvalidNode: rank(c) is the sorted rank of their canonical k-mer, or -1
template <class Rank>
uint32_t node_at(const Graph& g, const char* s, Rank&& rank) {
  int strand = 0;
  const int64_t r = with_kmer_type(g.kmer_bytes, [&](auto t) -> int64_t {
    typename decltype(t)::type c;
    encode_kmer(s, g.k, &c, &strand);
    return rank(c);
  });
  if (r < 0) return kInvalidNode;
  return 2 * g.rank2id[(size_t)r] + ((uint32_t)strand ^ (uint32_t)g.flip[(size_t)r]);
}

}  // namespace

uint32_t Graph::node_of(const char* s) const {
  if (n == 0 || num_sets() > 1) return kInvalidNode;
  return node_at(*this, s, [&](auto c) { return rank_of(*this, c); });
}

uint32_t Graph::node_of_in(uint32_t set, const char* s) const {
  if (set >= num_sets()) return kInvalidNode;
  if (set_lo.empty()) return node_of(s);
  const uint64_t lo = set_lo[set], hi = set_lo[(size_t)set + 1];
  if (lo == hi) return kInvalidNode;
  return node_at(*this, s, [&](auto c) { return rank_in(*this, lo, hi, c); });
}

std::string Graph::node_string(uint32_t v) const {
  const uint32_t r = id2rank[v >> 1];
  const int strand = (int)((v & 1u) ^ (uint32_t)flip[r]);
  return with_kmer_type(kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    return decode_kmer<KT>(kmer_vec<KT>(*this)[r], strand, k);
  });
}

SolidCountInfo last_solid_count() { return g_solid_info.get(); }

uint64_t graph_max_kmers() {
  const uint64_t cap = 1ull << 30;
  const char* s = getenv("G2S_BUILD_MAX_KMERS");
  const uint64_t v = s && *s ? strtoull(s, nullptr, 10) : 0;
  return v && v < cap ? v : cap;
}

namespace {

// The bounded set of a single graph on host threads (dbg.hpp: GraphReach; the device form is graph_reach.h): `keep`
// holds the sorted solid k-mers and leaves with those of them within reach of a seed.  One search for all records: level
// L's frontier is what level L - 1 claimed plus the seeds that enter at L = Rmax - their radius, one bit a solid k-mer
// marks what is visited, and a k-mer is claimed at the earliest level that reaches it — the one that leaves it the most
// budget — so that what is visited after level Rmax is the union of the records' balls.
template <class KT>
void reach_filter_host(std::vector<KT>& keep, const GraphReach& reach, int k, int nthreads, GraphReachInfo* info) {
  const ReachSeeds<KT> rs = make_reach_seeds<KT>(reach, k);
  const uint64_t n = keep.size();
  std::vector<std::atomic<uint64_t>> vis((size_t)(n / 64 + 1));
  for (auto& w : vis) w.store(0, std::memory_order_relaxed);
  auto find = [&](const KT& x) -> int64_t {
    auto it = std::lower_bound(keep.begin(), keep.end(), x);
    return (it != keep.end() && *it == x) ? (int64_t)(it - keep.begin()) : -1;
  };
  auto claim = [&](uint64_t i) { return !(vis[(size_t)(i >> 6)].fetch_or(1ull << (i & 63), std::memory_order_relaxed) & (1ull << (i & 63))); };
  const KT mask = KmerOps<KT>::mask(k);
  std::vector<uint64_t> frontier, next;
  std::vector<std::vector<uint64_t>> local((size_t)std::max(1, nthreads));
  uint64_t in_full = 0;
  uint32_t levels = 0;
  size_t cursor = 0;
  const auto t_search = std::chrono::steady_clock::now();
  for (uint32_t level = 0; level <= rs.rmax; level++) {
    uint64_t s0, s1;
    rs.at(level, &cursor, &s0, &s1);
    for (uint64_t s = s0; s < s1; s++) {
      const int64_t i = find(rs.key[(size_t)s]);
      if (i < 0) continue;
      in_full++;
      if (claim((uint64_t)i)) frontier.push_back((uint64_t)i);
    }
    if (frontier.empty()) {
      if (cursor == rs.entry.size()) break;  // (nothing enters later either)
      level = rs.entry[cursor] - 1;          // (on to the level at which seeds enter next)
      continue;
    }
    levels = level;
    if (level == rs.rmax) break;  // (the rim: claimed, not expanded)
    for (auto& l : local) l.clear();
    parallel_for(frontier.size(), nthreads, [&](uint64_t b, uint64_t e, int t) {
      std::vector<uint64_t>& out = local[(size_t)t];
      for (uint64_t f = b; f < e; f++) {
        const KT c = keep[(size_t)frontier[(size_t)f]], rc = KmerOps<KT>::revcomp(c, k);
        for (int strand = 0; strand < 2; strand++) {
          const KT seq = strand == 0 ? c : rc, rseq = strand == 0 ? rc : c;
          for (int nt = 0; nt < 4; nt++) {
            const KT y = ((seq << 2) | (KT)nt) & mask;
            const KT ry = (rseq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));
            const int64_t i = find(y < ry ? y : ry);
            if (i >= 0 && claim((uint64_t)i)) out.push_back((uint64_t)i);
          }
        }
      }
    });
    next.clear();
    for (auto& l : local) next.insert(next.end(), l.begin(), l.end());
    frontier.swap(next);
  }
  info->ms_search = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_search).count();
  std::vector<KT> kept;
  for (uint64_t i = 0; i < n; i++)
    if (vis[(size_t)(i >> 6)].load(std::memory_order_relaxed) >> (i & 63) & 1) kept.push_back(keep[(size_t)i]);
  info->seeds_in_full = in_full;
  info->full_kmers = n;
  info->kept_kmers = kept.size();
  info->levels = levels;
  info->on_device = 0;
  keep.swap(kept);
}

Graph* graph_build_from(const BuildInput& in, int k, int solid, int nthreads, std::string* err, bool* gave_up);
}  // namespace

GraphReachInfo last_graph_reach() { return g_graph_reach_info.get(); }
// dbg_gpu.hip: what the device form of the bounded build did
void set_graph_reach_info(const GraphReachInfo& info) { g_graph_reach_info.set(info); }

Graph* graph_build(const std::vector<std::pair<const char*, uint64_t>>& seqs, int k, int solid, int nthreads,
                   std::string* err, const GraphReach* reach) {
  BuildInput in;
  in.seqs = &seqs;
  in.reach = reach;
  return graph_build_from(in, k, solid, nthreads, err, nullptr);
}
Graph* graph_build_text(DeviceText* text, int k, int solid, int nthreads, std::string* err, bool* gave_up,
                        const GraphReach* reach) {
  BuildInput in;
  in.text = text;
  in.reach = reach;
  *gave_up = false;
  return graph_build_from(in, k, solid, nthreads, err, gave_up);
}

namespace {
Graph* graph_build_from(const BuildInput& in, int k, int solid, int nthreads, std::string* err, bool* gave_up) {
  if (k < 1 || k > kMaxK) { if (err) *err = "k must be in [1," + std::to_string(kMaxK) + "]"; return nullptr; }
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  Graph* g = new_graph(k, solid);
  g->bounded = in.reach != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  // the solid k-mer set: sort on the GPU when there is one (dbg_gpu.hip), host threads otherwise
  bool set_on_gpu = false;
  SolidCountInfo info;
  if (in.text) info.positions = in.text->T;
  else for (auto& sq : *in.seqs) info.positions += sq.second + 1;
  std::string why = "G2S_HOST_BUILD";
  if (!host_build_asked()) {
    set_on_gpu = count_solid_gpu(*g, in, solid, build_device(), &why, &info);
    if (!set_on_gpu && getenv("G2S_DEBUG")) fprintf(stderr, "[g2s]   k-mer set on the host (%s)\n", why.c_str());
  }
  if (!set_on_gpu && in.text) {  // (the host count reads sequences: the caller loads them on the host and comes back)
    if (err) *err = why;
    *gave_up = true;
    delete g;
    return nullptr;
  }
  if (!set_on_gpu) with_kmer_type(g->kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    count_solid<KT>(*g, *in.seqs, solid, nthreads);
    if (in.reach) {  // the same search as the device's, over the sorted vector
      GraphReachInfo ri;
      ri.records = in.reach->records;
      ri.seeds = in.reach->seed.size();
      reach_filter_host<KT>(kmer_vec<KT>(*g), *in.reach, k, nthreads, &ri);
      g->n = ri.kept_kmers;
      if (getenv("G2S_DEBUG"))
        fprintf(stderr, "[g2s]   reach: %llu of %llu k-mers kept on the host, %u levels\n", (unsigned long long)ri.kept_kmers,
                (unsigned long long)ri.full_kmers, ri.levels);
      set_graph_reach_info(ri);
    }
  });
  const auto t1 = std::chrono::steady_clock::now();
  if (!set_on_gpu) info.passes = info.refined_bins = 0, info.max_pass_keys = 0;
  info.on_device = set_on_gpu ? 1 : 0;
  info.solid = g->n;
  g_solid_info.set(info);
  const std::string how = !set_on_gpu ? "host" : info.passes ? "GPU, " + std::to_string(info.passes) + " key-range passes" : "GPU sort";
  if (g->n >= graph_max_kmers()) { if (err) *err = kTooManyKmers; delete g; return nullptr; }
  with_kmer_type(g->kmer_bytes, [&](auto t) { finish_graph<typename decltype(t)::type>(*g, nthreads); });
  if (getenv("G2S_DEBUG"))
    fprintf(stderr, "[g2s] graph build: %llu k-mers; solid k-mer set %.3f s (%s), tables + unitig order %.3f s (%d threads)\n",
            (unsigned long long)g->n, std::chrono::duration<double>(t1 - t0).count(), how.c_str(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count(), nthreads);
  return g;
}
}  // namespace

namespace {

// One set's graph on one host thread (a small prefix index: sets are small), appended to the union at ranks and node
// indices [off, off + n_s).
template <class KT>
void build_set_part(const std::vector<std::pair<const char*, uint64_t>>& seqs, int solid, Graph* part) {
  count_solid<KT>(*part, seqs, solid, 1);
  int bits = 1;
  while (bits < 22 && (1ull << bits) < part->n) bits++;
  build_bucket_index<KT>(*part, bits);
  finish_graph_host<KT>(*part, 1);
}

template <class KT>
void append_set_part(Graph& u, const Graph& p, uint64_t off) {
  std::vector<KT>& uk = kmer_vec<KT>(u);
  const std::vector<KT>& pk = kmer_vec<KT>(p);
  std::copy(pk.begin(), pk.end(), uk.begin() + (ptrdiff_t)off);
  const uint32_t o = (uint32_t)off;
  for (uint64_t r = 0; r < p.n; r++) {
    u.rank2id[(size_t)(off + r)] = p.rank2id[(size_t)r] + o;
    u.id2rank[(size_t)(off + r)] = p.id2rank[(size_t)r] + o;
    u.flip[(size_t)(off + r)] = p.flip[(size_t)r];
  }
  for (size_t q = 0; q < p.succ.size(); q++) u.succ[(size_t)off * 8 + q] = p.succ[q] == kInvalidNode ? kInvalidNode : p.succ[q] + 2 * o;
  for (size_t q = 0; q < p.pred.size(); q++) u.pred[(size_t)off * 8 + q] = p.pred[q] == kInvalidNode ? kInvalidNode : p.pred[q] + 2 * o;
  std::copy(p.lastnt.begin(), p.lastnt.end(), u.lastnt.begin() + (ptrdiff_t)(2 * off));
}

using SetSeqsFn = std::function<const std::vector<std::pair<const char*, uint64_t>>*(uint32_t, std::vector<std::pair<const char*, uint64_t>>*)>;
// (own_part(s, mine, part): true when it built set s's part itself — a set with a reach record)
using SetPartFn = std::function<bool(uint32_t, const std::vector<std::pair<const char*, uint64_t>>&, Graph*)>;
Graph* build_sets_host(const SetSeqsFn& set_seqs, uint32_t nsets, int k, int solid, int nthreads,
                       std::chrono::steady_clock::time_point t0, std::string* err, const SetPartFn* own_part = nullptr);

}  // namespace

Graph* graph_build_sets(const std::vector<std::pair<const char*, uint64_t>>& seqs, const std::vector<uint32_t>& seq_set,
                        uint32_t nsets, int k, int solid, int nthreads, std::string* err) {
  if (k < 1 || k > kMaxK) { if (err) *err = "k must be in [1," + std::to_string(kMaxK) + "]"; return nullptr; }
  if (nsets == 0 || seq_set.size() != seqs.size()) { if (err) *err = "graph_build_sets: no sets, or a set id per sequence missing"; return nullptr; }
  for (uint32_t s : seq_set)
    if (s >= nsets) { if (err) *err = "graph_build_sets: set id " + std::to_string(s) + " out of range"; return nullptr; }
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  const auto t0 = std::chrono::steady_clock::now();
  // on the GPU when there is one (dbg_gpu.hip: keyed k-mer sort, successors searched inside their set); no device,
  // G2S_HOST_BUILD=1, an empty union: the host build below, set by set
  if (Graph* g = build_on_device(k, solid, "set graph", [&](Graph& dg, int device, const HostWalk& walk, std::string* why) {
        return graph_build_sets_gpu(dg, seqs, seq_set, nsets, solid, device, walk, why);
      })) {
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s] set graph build: %u sets, %llu k-mers, %.3f s on the GPU\n", nsets, (unsigned long long)g->n,
              std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return g;
  }
  std::vector<std::vector<std::pair<const char*, uint64_t>>> by_set(nsets);
  for (size_t j = 0; j < seqs.size(); j++) by_set[seq_set[j]].push_back(seqs[j]);
  return build_sets_host([&](uint32_t s, std::vector<std::pair<const char*, uint64_t>>* tmp) { (void)tmp; return &by_set[s]; }, nsets, k,
                         solid, nthreads, t0, err);
}

namespace {

// The set graph on host threads, set by set: set_seqs(s, tmp) gives set s's (pointer, length) list (its own, or one
// written into tmp, a list of the calling thread).
Graph* build_sets_host(const SetSeqsFn& set_seqs, uint32_t nsets, int k, int solid, int nthreads,
                       std::chrono::steady_clock::time_point t0, std::string* err, const SetPartFn* own_part) {
  const int kb = kmer_width(k);
  std::vector<Graph*> parts(nsets, nullptr);
  {
    std::atomic<uint32_t> next(0);
    auto work = [&]() {
      std::vector<std::pair<const char*, uint64_t>> tmp;
      while (true) {
        const uint32_t s = next.fetch_add(1);
        if (s >= nsets) break;
        Graph* p = new_graph(k, solid);
        const std::vector<std::pair<const char*, uint64_t>>& mine = *set_seqs(s, &tmp);
        if (!(own_part && (*own_part)(s, mine, p)))
          with_kmer_type(kb, [&](auto t) { build_set_part<typename decltype(t)::type>(mine, solid, p); });
        parts[s] = p;
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < std::min<int>(nthreads, (int)nsets); t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
  }
  Graph* g = new_graph(k, solid);
  g->set_lo.assign((size_t)nsets + 1, 0);
  for (uint32_t s = 0; s < nsets; s++) {
    g->set_lo[(size_t)s + 1] = g->set_lo[s] + parts[s]->n;
    g->n_unitigs += parts[s]->n_unitigs;
  }
  g->n = g->set_lo[nsets];
  if (g->n >= (1ull << 30)) {  // (not graph_max_kmers(): G2S_BUILD_MAX_KMERS bounds single graphs, not set graphs)
    if (err) *err = kTooManyKmers;
    for (Graph* p : parts) delete p;
    delete g;
    return nullptr;
  }
  with_kmer_type(kb, [&](auto t) { kmer_vec<typename decltype(t)::type>(*g).resize((size_t)g->n); });
  g->rank2id.assign((size_t)g->n, 0);
  g->id2rank.assign((size_t)g->n, 0);
  g->flip.assign((size_t)g->n, 0);
  g->succ.assign((size_t)g->n * 8, kInvalidNode);
  if (k % 2 == 0) g->pred.assign((size_t)g->n * 8, kInvalidNode);
  g->lastnt.assign((size_t)g->n * 2, 0);
  parallel_for(nsets, std::min(nthreads, 16), [&](uint64_t b, uint64_t e, int) {
    for (uint64_t s = b; s < e; s++) {
      with_kmer_type(kb, [&](auto t) { append_set_part<typename decltype(t)::type>(*g, *parts[s], g->set_lo[s]); });
      delete parts[s];
      parts[s] = nullptr;
    }
  });
  build_ustart(*g);
  if (getenv("G2S_DEBUG"))
    fprintf(stderr, "[g2s] set graph build: %u sets, %llu k-mers, %.3f s on the host (%d threads)\n", nsets,
            (unsigned long long)g->n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), nthreads);
  return g;
}

}  // namespace

PoolBuildInfo last_pool_build() { return g_pool_info.get(); }

static bool check_pool_sets(const PoolSets& ps, int k, std::string* err) {
  if (k < 1 || k > kMaxK) { if (err) *err = "k must be in [1," + std::to_string(kMaxK) + "]"; return false; }
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  if (ps.nsets == 0 || seqs.size() >= (1ull << 32)) { if (err) *err = "graph_build_pool: no sets, or 2^32 sequences or more"; return false; }
  for (uint32_t s = 0; s < ps.nsets; s++)
    if (ps.set_begin[s + 1] < ps.set_begin[s]) { if (err) *err = "graph_build_pool: set_begin decreases at set " + std::to_string(s); return false; }
  for (uint64_t q = ps.set_begin[0]; q < ps.set_begin[ps.nsets]; q++)
    if (ps.set_seq[q] >= seqs.size()) { if (err) *err = "graph_build_pool: sequence index " + std::to_string(ps.set_seq[q]) + " out of range"; return false; }
  for (uint64_t x = 0; x < ps.nshared; x++)
    if (ps.shared_seq[x] >= seqs.size()) { if (err) *err = "graph_build_pool: shared sequence index " + std::to_string(ps.shared_seq[x]) + " out of range"; return false; }
  return true;
}

// the positions (bases + 1) of the pool's sequences some list names, once each: what the host build reads as host text
static uint64_t pool_text_in_use(const PoolSets& ps) {
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  std::vector<uint8_t> seen(seqs.size(), 0);
  uint64_t n = 0, flagged = 0;
  auto use = [&](uint32_t j) { if (!seen[j]) { seen[j] = 1; n += seqs[j].second + 1; } };
  for (uint64_t q = ps.set_begin[0]; q < ps.set_begin[ps.nsets]; q++) use(ps.set_seq[q]);
  for (uint32_t s = 0; s < ps.nsets; s++) flagged += ps.flagged(s) ? 1 : 0;
  for (uint64_t x = 0; flagged && x < ps.nshared; x++) use(ps.shared_seq[x]);
  return n;
}

// set s's list into *out, its own sequences and behind them the shared list's when `with_shared`: pointers only, no text moves
static std::vector<std::pair<const char*, uint64_t>>* expand_set(const PoolSets& ps, uint32_t s, bool with_shared,
                                                                 std::vector<std::pair<const char*, uint64_t>>* out) {
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  out->clear();
  for (uint64_t q = ps.set_begin[s]; q < ps.set_begin[s + 1]; q++) out->push_back(seqs[ps.set_seq[q]]);
  if (with_shared)
    for (uint64_t x = 0; x < ps.nshared; x++) out->push_back(seqs[ps.shared_seq[x]]);
  return out;
}

// What the host route of a pooled build does, of its flagged sets `whole` built from their expanded lists and `bounded`
// from reach records: those read the shared list through one table, sorted once for all of them.
static PoolBuildInfo pool_info_host(const PoolSets& ps, uint64_t whole, uint64_t bounded) {
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  PoolBuildInfo info;
  info.text_packed = pool_text_in_use(ps);
  for (uint64_t q = ps.set_begin[0]; q < ps.set_begin[ps.nsets]; q++) info.own_positions += seqs[ps.set_seq[q]].second + 1;
  if (whole + bounded)
    for (uint64_t x = 0; x < ps.nshared; x++) info.shared_positions += seqs[ps.shared_seq[x]].second + 1;
  info.keys_sorted = info.own_positions + (whole + (bounded ? 1 : 0)) * info.shared_positions;
  return info;
}

Graph* graph_build_pool(const PoolSets& ps, int k, int solid, int nthreads, std::string* err) {
  if (!check_pool_sets(ps, k, err)) return nullptr;
  if (ps.nsets == 1) {  // an ordinary graph, as graph_build_sets' callers get for one set
    std::vector<std::pair<const char*, uint64_t>> all;
    if (ps.host_text && !ps.host_text(err)) return nullptr;  // (graph_build takes host pointers)
    Graph* g1 = graph_build(*expand_set(ps, 0, ps.flagged(0), &all), k, solid, nthreads, err);
    if (g1)  // (no pooled build ran: the text counters alone change)
      g_pool_info.update([&](PoolBuildInfo& last) {
        last.text_gathered = 0;
        last.text_packed = pool_text_in_use(ps);
      });
    return g1;
  }
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  const auto t0 = std::chrono::steady_clock::now();
  PoolBuildInfo info;
  // on the GPU when there is one (dbg_gpu.hip: the pool's k-mers extracted once, the own lists' (set, k-mer) pairs and
  // the shared list's k-mers gathered from them, the shared list sorted once and merged into every flagged set); no
  // device, G2S_HOST_BUILD=1, an empty union: the host build, set by set over each set's pointers
  if (Graph* g = build_on_device(k, solid, "pooled set graph", [&](Graph& dg, int device, const HostWalk& walk, std::string* why) {
        return graph_build_pool_gpu(dg, ps, solid, device, walk, &info, why);
      })) {
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s] pooled set graph build: %u sets, %llu k-mers, %llu own + %llu shared positions, %llu keys sorted, %.3f s on the GPU\n",
              ps.nsets, (unsigned long long)g->n, (unsigned long long)info.own_positions, (unsigned long long)info.shared_positions,
              (unsigned long long)info.keys_sorted, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    info.on_device = 1;
    g_pool_info.set(info);
    return g;
  }
  if (ps.host_text && !ps.host_text(err)) return nullptr;
  uint64_t flagged = 0;
  for (uint32_t s = 0; s < ps.nsets; s++) flagged += ps.flagged(s) ? 1 : 0;
  info = pool_info_host(ps, flagged, 0);
  Graph* g = build_sets_host([&](uint32_t s, std::vector<std::pair<const char*, uint64_t>>* tmp) { return expand_set(ps, s, ps.flagged(s), tmp); },
                             ps.nsets, k, solid, nthreads, t0, err);
  if (g) g_pool_info.set(info);
  return g;
}

// ---- pooled set graphs bounded by reach records (dbg.hpp: PoolReach) ---------------------------------
namespace {

template <class KT>
struct KmerHasher {
  size_t operator()(const KT& x) const { return (size_t)KmerOps<KT>::hash(x); }
};

// the canonical k-mers of a list of sequences as a sorted (k-mer, copies) table
template <class KT>
struct CountTable {
  std::vector<KT> key;
  std::vector<uint32_t> cnt;
  void build(const std::vector<std::pair<const char*, uint64_t>>& seqs, int k) {
    std::vector<KT> all;
    for (auto& s : seqs) {
      KmerRoller<KT> r(k);
      for (uint64_t i = 0; i < s.second; i++)
        if (r.push(s.first[i])) all.push_back(r.canonical());
    }
    std::sort(all.begin(), all.end());
    for (size_t i = 0; i < all.size();) {
      size_t j = i + 1;
      while (j < all.size() && all[j] == all[i]) j++;
      key.push_back(all[i]);
      cnt.push_back((uint32_t)std::min<size_t>(j - i, 0xFFFFFFFFu));
      i = j;
    }
  }
  uint64_t count(const KT& x) const {
    auto it = std::lower_bound(key.begin(), key.end(), x);
    return (it != key.end() && *it == x) ? cnt[(size_t)(it - key.begin())] : 0;
  }
};

// One set with a reach record on one host thread: a breadth-first search from the seeds over the implicit full graph
// (a k-mer is in it when its copies in the own table and, for a flagged set, in the shared table reach `solid`); the
// full graph is never formed.  full != nullptr: its k-mers are counted (a pass over the two tables).
template <class KT>
void build_reach_part(const std::vector<std::pair<const char*, uint64_t>>& own_seqs, const CountTable<KT>* shared,
                      const char* const* seeds, uint64_t nseeds, int32_t radius, int k, int solid, Graph* part, uint64_t* full,
                      uint32_t* levels) {
  const uint64_t so = (uint64_t)std::max(1, solid);
  CountTable<KT> own;
  own.build(own_seqs, k);
  auto member = [&](const KT& x) { return own.count(x) + (shared ? shared->count(x) : 0) >= so; };
  std::unordered_set<KT, KmerHasher<KT>> seen;
  std::vector<KT> frontier, next;
  for (uint64_t i = 0; i < nseeds; i++) {
    KT c;
    int strand;
    encode_kmer<KT>(seeds[i], k, &c, &strand);
    if (member(c) && seen.insert(c).second) frontier.push_back(c);
  }
  const KT mask = KmerOps<KT>::mask(k);
  uint32_t level = 0;
  while (!frontier.empty() && (int64_t)level < (int64_t)radius) {
    next.clear();
    for (const KT& c : frontier) {
      const KT rc = KmerOps<KT>::revcomp(c, k);
      for (int strand = 0; strand < 2; strand++) {
        const KT seq = strand == 0 ? c : rc, rseq = strand == 0 ? rc : c;
        for (int nt = 0; nt < 4; nt++) {
          const KT y = ((seq << 2) | (KT)nt) & mask;
          const KT ry = (rseq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));
          const KT x = y < ry ? y : ry;
          if (seen.count(x) || !member(x)) continue;
          seen.insert(x);
          next.push_back(x);
        }
      }
    }
    if (next.empty()) break;
    level++;
    frontier.swap(next);
  }
  *levels = level;
  std::vector<KT>& keep = kmer_vec<KT>(*part);
  keep.assign(seen.begin(), seen.end());
  std::sort(keep.begin(), keep.end());
  part->n = keep.size();
  if (full) {
    uint64_t f = 0;
    for (size_t i = 0; i < own.key.size(); i++) f += member(own.key[i]) ? 1 : 0;
    if (shared)
      for (size_t u = 0; u < shared->key.size(); u++)
        if (shared->cnt[u] >= so && own.count(shared->key[u]) == 0) f++;
    *full = f;
  }
  int bits = 1;
  while (bits < 22 && (1ull << bits) < part->n) bits++;
  build_bucket_index<KT>(*part, bits);
  finish_graph_host<KT>(*part, 1);
}

template <class KT>
Graph* build_pool_reach_host(const PoolSets& ps, const PoolReach& reach, int k, int solid, int nthreads, bool count_full,
                             std::chrono::steady_clock::time_point t0, PoolReachInfo* rinfo, std::string* err) {
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  CountTable<KT> shared;  // built once, for the flagged sets with a record
  bool want_shared = false;
  for (uint32_t s = 0; s < ps.nsets; s++) want_shared = want_shared || (reach.has(s) && ps.flagged(s));
  if (want_shared) {
    std::vector<std::pair<const char*, uint64_t>> sh;
    for (uint64_t x = 0; x < ps.nshared; x++) sh.push_back(seqs[ps.shared_seq[x]]);
    shared.build(sh, k);
  }
  std::vector<uint64_t> full(ps.nsets, 0), kept(ps.nsets, 0);
  std::vector<uint32_t> levels(ps.nsets, 0);
  const SetPartFn own_part = [&](uint32_t s, const std::vector<std::pair<const char*, uint64_t>>&, Graph* part) -> bool {
    if (!reach.has(s)) return false;
    std::vector<std::pair<const char*, uint64_t>> own;
    build_reach_part<KT>(*expand_set(ps, s, false, &own), ps.flagged(s) ? &shared : nullptr, reach.seed.data() + reach.seed_begin[s],
                         reach.seed_begin[s + 1] - reach.seed_begin[s], reach.radius[s], k, solid, part,
                         count_full ? &full[s] : nullptr, &levels[s]);
    kept[s] = part->n;
    return true;
  };
  Graph* g = build_sets_host([&](uint32_t s, std::vector<std::pair<const char*, uint64_t>>* tmp) {
    if (reach.has(s)) { tmp->clear(); return tmp; }  // (own_part reads the lists itself)
    return expand_set(ps, s, ps.flagged(s), tmp);
  }, ps.nsets, k, solid, nthreads, t0, err, &own_part);
  for (uint32_t s = 0; s < ps.nsets; s++) {
    if (!reach.has(s)) continue;
    rinfo->reach_sets++;
    rinfo->full_kmers += full[s];
    rinfo->kept_kmers += kept[s];
    rinfo->levels = std::max(rinfo->levels, levels[s]);
  }
  rinfo->full_known = count_full ? 1 : 0;
  rinfo->on_device = 0;
  return g;
}

// a graph of one set as the ordinary graph the pooled builds give for nsets == 1
template <class KT>
void collapse_to_one_set(Graph& g) {
  g.set_lo.clear();
  build_bucket_index<KT>(g);
}

}  // namespace

PoolReachInfo last_pool_reach() { return g_reach_info.get(); }

Graph* graph_build_pool_reach(const PoolSets& ps_in, const PoolReach& reach_in, int k, int solid, int nthreads, std::string* err) {
  if (!reach_in.any()) return graph_build_pool(ps_in, k, solid, nthreads, err);
  if (!check_pool_sets(ps_in, k, err)) return nullptr;
  if (reach_in.radius.size() != ps_in.nsets || reach_in.seed_begin.size() != (size_t)ps_in.nsets + 1) {
    if (err) *err = "graph_build_pool_reach: a reach record per set missing";
    return nullptr;
  }
  // one set: built as two (the second empty, without a record) and handed back as an ordinary graph
  PoolSets ps = ps_in;
  PoolReach reach1;
  std::vector<uint64_t> begin2;
  std::vector<uint8_t> shared2;
  const bool one = ps_in.nsets == 1;
  if (one) {
    begin2 = {ps_in.set_begin[0], ps_in.set_begin[1], ps_in.set_begin[1]};
    shared2 = {(uint8_t)(ps_in.flagged(0) ? 1 : 0), 0};
    ps.set_begin = begin2.data();
    ps.set_shared = shared2.data();
    ps.nsets = 2;
    reach1 = reach_in;
    reach1.radius.push_back(-1);
    reach1.seed_begin.push_back(reach1.seed_begin.back());
  }
  const PoolReach& reach = one ? reach1 : reach_in;
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  const auto t0 = std::chrono::steady_clock::now();
  const int kb = kmer_width(k);
  PoolBuildInfo info;
  PoolReachInfo rinfo;
  bool device_gave_up = false;  // (the device build got as far as selecting the device — not a machine without one)
  Graph* g = build_on_device(k, solid, "pooled set graph", [&](Graph& dg, int device, const HostWalk& walk, std::string* why) {
    return graph_build_pool_gpu(dg, ps, solid, device, walk, &info, why, &reach, &rinfo, &device_gave_up);
  });
  if (g) {
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s] pooled set graph build: %u sets, %llu k-mers, %llu own + %llu shared positions, %llu keys sorted, %.3f s on the GPU; "
                      "reach: %llu sets, %llu k-mers kept, %u levels\n",
              ps_in.nsets, (unsigned long long)g->n, (unsigned long long)info.own_positions, (unsigned long long)info.shared_positions,
              (unsigned long long)info.keys_sorted, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
              (unsigned long long)rinfo.reach_sets, (unsigned long long)rinfo.kept_kmers, rinfo.levels);
    info.on_device = 1;
  } else {
    if (ps.host_text && !ps.host_text(err)) return nullptr;
    uint64_t whole = 0, bounded = 0;  // flagged sets without / with a record
    for (uint32_t s = 0; s < ps.nsets; s++)
      if (ps.flagged(s)) (reach.has(s) ? bounded : whole)++;
    info = pool_info_host(ps, whole, bounded);
    rinfo = PoolReachInfo();
    g = with_kmer_type(kb, [&](auto t) {
      return build_pool_reach_host<typename decltype(t)::type>(ps, reach, k, solid, nthreads, !device_gave_up, t0, &rinfo, err);
    });
    if (!g) return nullptr;
  }
  if (one) with_kmer_type(kb, [&](auto t) { collapse_to_one_set<typename decltype(t)::type>(*g); });
  g_pool_info.set(info);
  g_reach_info.set(rinfo);
  return g;
}

// ---- own cache format ------------------------------------------------------
static const char kMagic[8] = {'G', '2', 'S', 'D', 'B', 'G', '0', '2'};

bool graph_save(const Graph& g, const std::string& path, std::string* err) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  // (header word 3: bit 0 = explicit predecessor table, bits 8.. = the abundance threshold of the set)
  uint64_t hdr[4] = {(uint64_t)g.k, g.n, g.n_unitigs, (uint64_t)(g.pred.empty() ? 0 : 1) | ((uint64_t)std::max(0, g.solid) << 8)};
  bool ok = fwrite(kMagic, 1, 8, f) == 8 && fwrite(hdr, 8, 4, f) == 4;
  auto put = [&](const void* p, size_t bytes) { if (ok && bytes) ok = fwrite(p, 1, bytes, f) == bytes; };
  // (the width follows from k: 8-, 16- or 32-byte k-mers, little-endian words, least significant first)
  with_kmer_type(g.kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    put(kmer_vec<KT>(g).data(), kmer_vec<KT>(g).size() * sizeof(KT));
  });
  put(g.rank2id.data(), g.rank2id.size() * 4);
  put(g.flip.data(), g.flip.size());
  put(g.succ.data(), g.succ.size() * 4);
  put(g.pred.data(), g.pred.size() * 4);
  put(g.lastnt.data(), g.lastnt.size());
  fclose(f);
  if (!ok && err) *err = "short write to " + path;
  return ok;
}

Graph* graph_load(const std::string& path, std::string* err) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return nullptr; }
  char magic[8];
  uint64_t hdr[4];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, kMagic, 8) != 0 || fread(hdr, 8, 4, f) != 4) {
    fclose(f);
    if (err) *err = "not a g2s graph cache: " + path;
    return nullptr;
  }
  // the file is not trusted: every size and index is checked before it is used
  const uint64_t solid_of_cache = hdr[3] >> 8;
  hdr[3] &= 0xFFull;
  if (hdr[0] < 1 || hdr[0] > (uint64_t)kMaxK || hdr[1] >= (1ull << 30) || hdr[2] > hdr[1] || hdr[3] > 1 || solid_of_cache > (1ull << 30)) {
    fclose(f);
    if (err) *err = "corrupt graph cache header: " + path;
    return nullptr;
  }
  {
    const uint64_t per = (uint64_t)kmer_width((int)hdr[0]) + 4u + 1u + 32u + (hdr[3] ? 32u : 0u) + 2u;
    const long here = ftell(f);
    fseek(f, 0, SEEK_END);
    const long end = ftell(f);
    fseek(f, here, SEEK_SET);
    if (here < 0 || end < 0 || (uint64_t)(end - here) != per * hdr[1]) {
      fclose(f);
      if (err) *err = "graph cache has the wrong size for its header: " + path;
      return nullptr;
    }
  }
  Graph* g = new Graph();
  g->k = (int)hdr[0];
  g->solid = (int)solid_of_cache;
  g->n = hdr[1];
  g->n_unitigs = hdr[2];
  g->kmer_bytes = kmer_width(g->k);
  bool ok = true;
  auto get = [&](void* p, size_t bytes) { if (ok && bytes) ok = fread(p, 1, bytes, f) == bytes; };
  with_kmer_type(g->kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    kmer_vec<KT>(*g).resize((size_t)g->n);
    get(kmer_vec<KT>(*g).data(), (size_t)g->n * sizeof(KT));
  });
  g->rank2id.resize((size_t)g->n); get(g->rank2id.data(), (size_t)g->n * 4);
  g->flip.resize((size_t)g->n); get(g->flip.data(), (size_t)g->n);
  g->succ.resize((size_t)g->n * 8); get(g->succ.data(), (size_t)g->n * 32);
  if (hdr[3]) { g->pred.resize((size_t)g->n * 8); get(g->pred.data(), (size_t)g->n * 32); }
  g->lastnt.resize((size_t)g->n * 2); get(g->lastnt.data(), (size_t)g->n * 2);
  fclose(f);
  if (!ok) { if (err) *err = "truncated graph cache: " + path; delete g; return nullptr; }
  auto corrupt = [&](const char* what) -> Graph* {
    if (err) *err = std::string("corrupt graph cache (") + what + "): " + path;
    delete g;
    return nullptr;
  };
  // sorted k-mer set, rank2id a permutation, neighbour ids in range, codes 0..3
  const bool ascending = with_kmer_type(g->kmer_bytes, [&](auto t) {
    const auto& v = kmer_vec<typename decltype(t)::type>(*g);
    for (size_t r = 1; r < v.size(); r++)
      if (!(v[r - 1] < v[r])) return false;
    return true;
  });
  if (!ascending) return corrupt("k-mers not strictly ascending");
  g->id2rank.assign((size_t)g->n, kInvalidNode);
  for (uint64_t r = 0; r < g->n; r++) {
    const uint32_t id = g->rank2id[(size_t)r];
    if (id >= g->n || g->id2rank[id] != kInvalidNode) return corrupt("rank2id is not a permutation");
    g->id2rank[id] = (uint32_t)r;
  }
  for (uint32_t w : g->succ) if (w != kInvalidNode && w >= 2 * g->n) return corrupt("successor out of range");
  for (uint32_t w : g->pred) if (w != kInvalidNode && w >= 2 * g->n) return corrupt("predecessor out of range");
  for (uint8_t c : g->lastnt) if (c > 3) return corrupt("base code out of range");
  for (uint8_t c : g->flip) if (c > 1) return corrupt("strand flag out of range");
  with_kmer_type(g->kmer_bytes, [&](auto t) { build_bucket_index<typename decltype(t)::type>(*g); });
  build_ustart(*g);
  return g;
}

}  // namespace g2s
