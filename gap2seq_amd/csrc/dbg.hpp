// gap2seq_amd/csrc/dbg.hpp — host-side de Bruijn graph: exact solid k-mer set,
// unitig-ordered node numbering and the 4-slot oriented successor table that is
// uploaded to HBM.
//
// Replaces gatb Graph::create / Graph::load as used at
// /root/reference/src/Gap2Seq.cpp:193-219 and the neighbour primitives
// Graph::successors / predecessors / contains / buildNode / toString whose call
// sites are Gap2Seq.cpp:879,884,924,955,957,995,1000,1043,1084,1086,1114,1199,
// 1203,1204,1263,1271,1452,1456,1476.  Membership is exact (no Bloom filter).
#pragma once
#include <algorithm>
#include <mutex>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <functional>
#include <string>
#include <vector>

#include "kmer.hpp"

namespace g2s {

static const uint32_t kInvalidNode = 0xFFFFFFFFu;
static const uint32_t kUstartPad = 64;  // 64-bit words of all-ones padding on either side of the device bitmap

struct DeviceGraph {
  uint32_t* succ = nullptr;  // [2n*4]
  uint32_t* pred = nullptr;  // [2n*4], only when k is even (palindromic k-mers exist); the device build leaves its own here
  uint64_t* ustart = nullptr;  // unitig-start bitmap, offset by kUstartPad words of all-ones padding
  uint32_t* rem = nullptr;     // [2n] unitig-internal steps left from an oriented node (seg_tables.hip)
  uint32_t* urec = nullptr;    // [2n][8] successor record of the end of the node's unitig walk + rem (seg_tables.hip)
  uint32_t* brec = nullptr;    // [2n][8] the same for walks backwards, only beside pred (seg_tables.h); odd k: urec serves
  // what the segment tier's kernels walk backwards with, and where they read a node's predecessors in slot order
  const uint32_t* back_table() const { return brec ? brec : urec; }
  uint64_t bytes = 0;
};

struct Graph {
  int k = 0;
  int solid = 0;      // abundance threshold the set was built with (0: unknown, a cache written before it was recorded)
  int kmer_bytes = 8; // k-mer width: 8 (k <= 31), 16 (k <= 63) or 32 bytes (k <= 127); kmer_width(k)
  uint64_t n = 0;     // canonical solid k-mers
  uint64_t n_unitigs = 0;
  bool bounded = false;  // built from reach records (GraphReach): the k-mers a gap list can reach, not the read set's
  // sorted canonical k-mers; exactly one of the three is used (the one of kmer_bytes)
  std::vector<uint64_t> kmers64;
  std::vector<u128> kmers128;
  std::vector<u256> kmers256;
  std::vector<uint32_t> bucket;   // prefix index over the sorted array
  int bucket_bits = 0;
  std::vector<uint32_t> rank2id;  // sorted rank -> node index (unitig order)
  std::vector<uint32_t> id2rank;
  // Orientation bit of an oriented node id is RELATIVE TO ITS UNITIG: bit 0 = the
  // direction in which the unitig was numbered.  flip[rank] = GATB strand
  // (0 = canonical) of that direction, so GATB strand = orientation ^ flip.  Inside a
  // unitig the only successor of an even id v is v+2 and of an odd id v is v-2, which
  // lets the kernels walk unitigs by arithmetic and verify in bulk.  GATB's strand is
  // only a label separating the two DP rows of a k-mer (Node::operator== ignores it),
  // so any consistent labelling gives identical results.
  std::vector<uint8_t> flip;
  // oriented node = 2*index + orientation.  succ[v*4 + nt] = oriented successor
  // obtained by appending nt (A,C,T,G) or kInvalidNode.
  std::vector<uint32_t> succ;
  std::vector<uint32_t> pred;     // explicit predecessor table, even k only
  std::vector<uint8_t> lastnt;    // [2n] code of the last base of the oriented sequence
  // The same as upper-case characters, one array per orientation ([n] each, by k-mer index): the bases along a
  // unitig are then consecutive bytes, and the traceback copies a run of states instead of looking every base
  // up (ensure_lastch builds them once, from lastnt).
  mutable std::vector<char> lastch_up, lastch_dn;
  mutable std::once_flag lastch_once;
  void ensure_lastch() const {
    std::call_once(lastch_once, [this]() {
      static const char kUpChar[4] = {'A', 'C', 'T', 'G'};  // GATB codes (kmer.hpp)
      lastch_up.resize((size_t)n);
      lastch_dn.resize((size_t)n);
      for (size_t i = 0; i < (size_t)n; i++) { lastch_up[i] = kUpChar[lastnt[2 * i] & 3]; lastch_dn[i] = kUpChar[lastnt[2 * i + 1] & 3]; }
    });
  }
  // bit i set: k-mer index i is the first of its unitig in numbering order, i.e. the edge
  // 2(i-1) -> 2i is NOT unitig-internal.  Between two set bits the walk arithmetic
  // (v +/- 2) is exact: every node there has exactly one predecessor and one successor.
  std::vector<uint64_t> ustart;
  std::map<int, DeviceGraph> dev; // per device copies
  // Set graphs (graph_build_sets): the disjoint union of one graph per read set, numbered set-major — set s holds
  // the node indices AND the sorted ranks [set_lo[s], set_lo[s+1]), its k-mers sorted within that range, no edge
  // leaves it.  Empty for a graph of one read set.
  std::vector<uint64_t> set_lo;
  uint32_t num_sets() const { return set_lo.empty() ? 1u : (uint32_t)(set_lo.size() - 1); }

  // buildNode + contains (kInvalidNode on a graph of several sets: a k-mer is a node of each set it is solid in)
  uint32_t node_of(const char* s) const;
  // ...restricted to one set's range
  uint32_t node_of_in(uint32_t set, const char* s) const;
  inline uint32_t succ_of(uint32_t v, int nt) const { return succ[(size_t)v * 4 + nt]; }
  // predecessor i in GATB order (prepend T,G,A,C)
  inline uint32_t pred_of(uint32_t v, int nt) const {
    if (!pred.empty()) return pred[(size_t)v * 4 + nt];
    uint32_t w = succ[(size_t)(v ^ 1u) * 4 + nt];
    return w == kInvalidNode ? w : (w ^ 1u);
  }
  std::string node_string(uint32_t v) const;
  inline char last_char(uint32_t v) const { return kNtChar[lastnt[v]]; }
};

static const int kMaxK = 127;
// bytes of the k-mer word for k in [1, kMaxK]
static inline int kmer_width(int k) { return k <= 31 ? 8 : k <= 63 ? 16 : 32; }
// The one dispatch on a k-mer width: f is called with a tag of the width's word and its result handed back, as in
//   with_kmer_type(g.kmer_bytes, [&](auto t) { using KT = typename decltype(t)::type; ... });
// A further width is added here, in kmer_vec below and in kmer_width alone.
template <class KT>
struct KmerTag { using type = KT; };
template <class F>
static inline auto with_kmer_type(int kmer_bytes, F&& f) {
  if (kmer_bytes == 8) return f(KmerTag<uint64_t>());
  if (kmer_bytes == 16) return f(KmerTag<u128>());
  return f(KmerTag<u256>());
}
// the graph's sorted k-mers as the vector of their width
template <class KT> std::vector<KT>& kmer_vec(Graph& g);
template <> inline std::vector<uint64_t>& kmer_vec<uint64_t>(Graph& g) { return g.kmers64; }
template <> inline std::vector<u128>& kmer_vec<u128>(Graph& g) { return g.kmers128; }
template <> inline std::vector<u256>& kmer_vec<u256>(Graph& g) { return g.kmers256; }
template <class KT> const std::vector<KT>& kmer_vec(const Graph& g);
template <> inline const std::vector<uint64_t>& kmer_vec<uint64_t>(const Graph& g) { return g.kmers64; }
template <> inline const std::vector<u128>& kmer_vec<u128>(const Graph& g) { return g.kmers128; }
template <> inline const std::vector<u256>& kmer_vec<u256>(const Graph& g) { return g.kmers256; }

// The device the graph builds and the reads loader run on: G2S_DEVICE, read on every call (it changes within a process).
static inline int build_device() {
  const char* s = getenv("G2S_DEVICE");
  return s ? atoi(s) : 0;
}
// What the process's last call of one kind did, for the test hooks to read: a value behind a mutex.
template <class T>
class LastInfo {
 public:
  T get() {
    std::lock_guard<std::mutex> lk(mu_);
    return v_;
  }
  void set(const T& v) { update([&](T& cur) { cur = v; }); }
  template <class F>
  void update(F&& f) {  // (some fields alone, under the lock)
    std::lock_guard<std::mutex> lk(mu_);
    f(v_);
  }

 private:
  std::mutex mu_;
  T v_;
};

struct GraphReach;
// seqs may contain any bytes; k-mers containing N/n are skipped (GATB model).  reach: BuildInput::reach.
Graph* graph_build(const std::vector<std::pair<const char*, uint64_t>>& seqs, int k, int solid, int nthreads,
                   std::string* err, const GraphReach* reach = nullptr);
// What the solid k-mer count reads: the caller's sequences, or a text that is already on a device (reads_text.h: every
// sequence followed by one 'N').  The device count frees a text as soon as it has read it for the last time.
struct DeviceText;
// Reach records of a single graph (g2s_graph_build_seqs_reach / _files_reach): the graph keeps, of the solid k-mers,
// those within radius[i] undirected steps of seed[i] for some i (k characters each, encoded as the fill's flank look-ups
// encode them; a seed outside the solid set is ignored).  One entry a seed: a record's seeds all carry its radius.
struct GraphReach {
  std::vector<const char*> seed;
  std::vector<int32_t> radius;  // [seed.size()], >= 0
  uint64_t records = 0;
};
struct BuildInput {
  const std::vector<std::pair<const char*, uint64_t>>* seqs = nullptr;
  DeviceText* text = nullptr;
  const GraphReach* reach = nullptr;  // the kept set instead of the full one (the cap applies to what is kept)
};
// The cap on a graph's k-mers (32-bit oriented node ids): 2^30, or G2S_BUILD_MAX_KMERS when that is lower (tests).
uint64_t graph_max_kmers();
static const char* const kTooManyKmers = "too many k-mers for 32-bit oriented node ids";
// The seeds of a bounded build as canonical k-mers in the order they enter the search: seed i at level
// Rmax - radius[i], so that a k-mer is claimed with the largest budget any record leaves it (graph_reach.h).
template <class KT>
struct ReachSeeds {
  std::vector<KT> key;            // sorted by entry level
  std::vector<uint32_t> entry;    // the distinct entry levels, ascending (sparse: a radius is bounded by int32 alone)
  std::vector<uint64_t> begin;    // [entry.size() + 1]: the seeds of level entry[j] are key[begin[j] .. begin[j + 1])
  uint32_t rmax = 0;
  // the seeds that enter at `level`, *cursor being the first entry level not yet taken (levels are asked for in order)
  void at(uint32_t level, size_t* cursor, uint64_t* s0, uint64_t* s1) const {
    *s0 = *s1 = 0;
    if (*cursor < entry.size() && entry[*cursor] == level) { *s0 = begin[*cursor]; *s1 = begin[*cursor + 1]; ++*cursor; }
  }
};
template <class KT>
static inline ReachSeeds<KT> make_reach_seeds(const GraphReach& reach, int k) {
  ReachSeeds<KT> rs;
  int32_t rmax = 0;
  for (int32_t r : reach.radius) rmax = r > rmax ? r : rmax;
  rs.rmax = (uint32_t)rmax;
  std::vector<std::pair<uint32_t, size_t>> order(reach.seed.size());  // (entry level, seed)
  for (size_t i = 0; i < reach.seed.size(); i++) order[i] = {(uint32_t)(rmax - reach.radius[i]), i};
  std::sort(order.begin(), order.end());
  rs.key.resize(order.size());
  for (size_t j = 0; j < order.size(); j++) {
    if (rs.entry.empty() || rs.entry.back() != order[j].first) { rs.entry.push_back(order[j].first); rs.begin.push_back(j); }
    int strand;
    encode_kmer<KT>(reach.seed[order[j].second], k, &rs.key[j], &strand);
  }
  rs.begin.push_back(order.size());
  return rs;
}
// What the process's last bounded single-graph build did (g2s_test_last_graph_reach).
struct GraphReachInfo {
  uint64_t records = 0, seeds = 0, seeds_in_full = 0, full_kmers = 0, kept_kmers = 0;
  uint32_t levels = 0, passes = 0, regrowths = 0;
  int on_device = 0;
  double ms_search = 0;  // the level loop alone (the last run of it, when the queue had to grow), wall time
};
GraphReachInfo last_graph_reach();
// graph_build from a text on a device.  Only the device count can read it: when that gives up (G2S_HOST_BUILD, no room,
// a HIP error) the result is nullptr with *gave_up set and the reason in *err, and the caller builds from the sequences.
// The text is the caller's to free either way (free_device_text: what the count has freed already is not freed twice).
Graph* graph_build_text(DeviceText* text, int k, int solid, int nthreads, std::string* err, bool* gave_up,
                        const GraphReach* reach = nullptr);
// What the process's last graph_build did for its solid k-mer set (g2s_test_last_solid_count): the text positions (bases
// + 1 a sequence), the key-range passes that ran (dbg_gpu.hip's pass form; 0: the one-sort device count, or the host), the
// histogram bins that had to be histogrammed again, the keys of the largest pass, the solid k-mers found, and whether the
// set was made on the device.
struct SolidCountInfo {
  uint64_t positions = 0, max_pass_keys = 0, solid = 0;
  uint32_t passes = 0, refined_bins = 0;
  int on_device = 0;
};
SolidCountInfo last_solid_count();
// One graph per read set, built on `nthreads` host threads (a set per thread at a time) and concatenated set-major
// (Graph::set_lo); seq_set[j] < nsets names the set of seqs[j].  Every set's part is what graph_build gives for its
// sequences alone, up to the numbering of nodes.
Graph* graph_build_sets(const std::vector<std::pair<const char*, uint64_t>>& seqs, const std::vector<uint32_t>& seq_set,
                        uint32_t nsets, int k, int solid, int nthreads, std::string* err);
// The same set graph from a POOL of sequences the sets share, without the expanded list: set s is the multiset
// seqs[set_seq[q]], q in [set_begin[s], set_begin[s+1]) (its own list), followed by seqs[shared_seq[*]] when
// set_shared[s] is set.  A sequence may be in any number of sets, and more than once in one; every occurrence counts
// towards solidity.  The graph is graph_build_sets' for the expanded list, up to the numbering of nodes inside a set.
// On the device (dbg_gpu.hip) the shared list is encoded and sorted once, whatever the number of flagged sets.
// A pool whose text lies in device memory (device_pool.h), for the sequences [first, first + n_reads) of PoolSets::seqs:
// every read followed by one 'N', read r at text + start[r] (start: device memory, n_reads + 1 entries).
struct PoolDeviceText {
  int device = -1;
  const uint8_t* text = nullptr;
  const uint64_t* start = nullptr;
  uint32_t first = 0;
  uint64_t n_reads = 0;
};
struct PoolSets {
  const std::vector<std::pair<const char*, uint64_t>>* seqs = nullptr;
  // g2s_graph_build_dpool_reach: a sequence whose pointer is null lies in one of these (sorted by `first`); the device
  // build gathers it from there (dbg_gpu.hip: k_gather_reads).  host_text() gives every such sequence a host pointer —
  // it is called once, in front of whatever reads the sequences on the host, and false fails the build with *err.
  const std::vector<PoolDeviceText>* device_text = nullptr;
  std::function<bool(std::string* err)> host_text;
  const uint64_t* set_begin = nullptr;   // [nsets + 1]
  const uint32_t* set_seq = nullptr;     // [set_begin[nsets]]
  const uint32_t* shared_seq = nullptr;  // [nshared]
  uint64_t nshared = 0;
  const uint8_t* set_shared = nullptr;   // [nsets], or nullptr: no set holds the shared list
  uint32_t nsets = 0;
  bool flagged(uint32_t s) const { return set_shared && set_shared[s] != 0; }
};
Graph* graph_build_pool(const PoolSets& ps, int k, int solid, int nthreads, std::string* err);
// What the process's last graph_build_pool of several sets did (g2s_test_last_pool_build): the positions (bases + 1 a
// sequence) of the own lists and of the shared list, and the keys that went through a sort — on the device
// own + shared whatever the number of flagged sets; the host build works on every flagged set's expanded list.
// text_gathered / text_packed (g2s_test_last_dpool): the positions of the sequences in use, once each, whose text the
// device build copied from a device-held pool / that went through host memory (the host build: all of them).
struct PoolBuildInfo {
  uint64_t own_positions = 0, shared_positions = 0, keys_sorted = 0;
  int on_device = 0;
  uint64_t text_gathered = 0, text_packed = 0;
};
PoolBuildInfo last_pool_build();
// Reach records of a pooled build (g2s_graph_build_pool_reach): set s with radius[s] >= 0 keeps, of its full graph, only
// the k-mers within radius[s] undirected steps (canonical k-mers, the eight neighbours of each) of one of its seeds —
// seed[seed_begin[s] .. seed_begin[s+1]), each k characters encoded as the fill's flank look-ups encode them
// (Graph::node_of_in).  A seed outside the full graph is ignored; a set whose seeds are all outside it is empty.
// radius[s] < 0: the whole set.
struct PoolReach {
  std::vector<int32_t> radius;        // [nsets]
  std::vector<uint64_t> seed_begin;   // [nsets + 1]
  std::vector<const char*> seed;      // [seed_begin[nsets]]
  bool has(uint32_t s) const { return s < radius.size() && radius[s] >= 0; }
  bool any() const { for (int32_t r : radius) if (r >= 0) return true; return false; }
};
Graph* graph_build_pool_reach(const PoolSets& ps, const PoolReach& reach, int k, int solid, int nthreads, std::string* err);
// What the process's last graph_build_pool_reach with a reach record did (g2s_test_last_pool_reach): the sets with a
// record, the k-mers of their full graphs (full_known == 0: not counted — the device build never forms them, and the
// host build does not count them behind a device build that gave up), the k-mers kept, the deepest level a set's
// search ran, and whether the search ran on the device.
struct PoolReachInfo {
  uint64_t reach_sets = 0, full_kmers = 0, kept_kmers = 0;
  int full_known = 0;
  uint32_t levels = 0;
  int on_device = 0;
};
PoolReachInfo last_pool_reach();
bool graph_save(const Graph& g, const std::string& path, std::string* err);
Graph* graph_load(const std::string& path, std::string* err);

}  // namespace g2s
