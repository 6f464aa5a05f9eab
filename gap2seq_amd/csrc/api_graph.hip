// gap2seq_amd/csrc/api_graph.hip — the C ABI's graph half (include/g2s.h): handles, the build entry points (sequences,
// read sets, pools, read files; reach records), save and load, node queries, upload, validation, and the test hooks
// that read the builders' info holders.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "api_internal.h"
#include "bam_reads.h"
#include "device_pool.h"
#include "fastx.hpp"
#include "pass_plan.hpp"
#include "readfilter_gaps.hpp"
#include "reads_text.h"

using namespace g2s;
using namespace g2s::api;

// ---------------------------------------------------------------------------
// graph
// ---------------------------------------------------------------------------

// what a builder of dbg.hpp made, handed back as a handle: null is the builder's refusal, with its reason in err
static int wrap_graph(Graph* g, const std::string& err, g2s_graph** out) {
  if (!g) return fail(G2S_ERR_ARG, err);
  *out = new g2s_graph();
  (*out)->g = g;
  return G2S_OK;
}
// the callers' sequences as (pointer, length) pairs; lens == nullptr: C strings
static std::vector<std::pair<const char*, uint64_t>> seq_pairs(const char* const* seqs, const uint64_t* lens, uint64_t n) {
  std::vector<std::pair<const char*, uint64_t>> v;
  v.reserve((size_t)n);
  for (uint64_t i = 0; i < n; i++) v.emplace_back(seqs[i], lens ? lens[i] : (uint64_t)strlen(seqs[i]));
  return v;
}

static int build_seqs_of(const char* const* seqs, const uint64_t* lens, int nseqs, int k, int solid, int nthreads,
                         const GraphReach* reach, g2s_graph** out) {
  if (!seqs || !out || nseqs < 0) return fail(G2S_ERR_ARG, "g2s_graph_build_seqs: bad argument");
  std::string err;
  return wrap_graph(graph_build(seq_pairs(seqs, lens, (uint64_t)nseqs), k, solid, nthreads, &err, reach), err, out);
}
extern "C" int g2s_graph_build_seqs(const char* const* seqs, const uint64_t* lens, int nseqs, int k, int solid,
                                    int nthreads, g2s_graph** out) {
  return build_seqs_of(seqs, lens, nseqs, k, solid, nthreads, nullptr, out);
}

// ---- single graphs bounded by reach records (include/g2s.h: g2s_graph_build_seqs_reach) --------------------
// A reach record's seeds: the flank k-mers the fill looks up (g2s_batch_prepare: the rule must match it), appended to
// *out.  False, and nothing appended, for a gap the fill rejects.
static bool flank_seeds(const g2s_gap& in, int k, std::vector<const char*>* out) {
  if (!in.left || !in.right || in.lmf < 0 || in.rmf < 0 || in.gap_len < 0 || in.left_len < k + in.lmf || in.right_len < k + in.rmf) return false;
  for (int x = 0; x <= in.lmf; x++) out->push_back(in.left + x);
  for (int x = 0; x <= in.rmf; x++) out->push_back(in.right + (in.right_len - k - x));
  for (int x = 0; x <= in.rmf; x++) out->push_back(in.right + x);
  return true;
}
// the records' seeds, one entry a seed with its record's radius
static int graph_reach_of(const char* name, int k, const g2s_gap* reach_gap, const int32_t* reach_radius, uint64_t nreach,
                          GraphReach* reach) {
  if (nreach && (!reach_gap || !reach_radius)) return fail(G2S_ERR_ARG, std::string(name) + ": reach_gap and reach_radius go together");
  if (k < 1 || k > kMaxK) return fail(G2S_ERR_ARG, "k must be in [1," + std::to_string(kMaxK) + "]");  // (the seeds read k characters)
  for (uint64_t r = 0; r < nreach; r++)
    if (reach_radius[r] < 0) return fail(G2S_ERR_ARG, std::string(name) + ": negative radius in record " + std::to_string(r));
  reach->records = nreach;
  for (uint64_t r = 0; r < nreach; r++)
    if (flank_seeds(reach_gap[r], k, &reach->seed)) reach->radius.resize(reach->seed.size(), reach_radius[r]);
  return G2S_OK;
}
// G2S_REACH_AUTO resolved: G2S_BUILD_REACH=1|0 overrides it; -1 for a mode that is none of the three
static int reach_mode_of(int mode) {
  if (mode != G2S_REACH_AUTO && mode != G2S_REACH_ALWAYS && mode != G2S_REACH_NEVER) return -1;
  const char* s = getenv("G2S_BUILD_REACH");
  if (mode == G2S_REACH_AUTO && s && *s) return strcmp(s, "0") != 0 ? G2S_REACH_ALWAYS : G2S_REACH_NEVER;
  return mode;
}
// plain(reach) is the build: with nullptr today's path.  AUTO runs that first and starts over on the cap error alone.
template <class Build>
static int build_with_reach(const char* name, int k, const g2s_gap* reach_gap, const int32_t* reach_radius, uint64_t nreach, int mode,
                            g2s_graph** out, Build&& build) {
  if (!out) return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
  mode = reach_mode_of(mode);
  if (mode < 0) return fail(G2S_ERR_ARG, std::string(name) + ": unknown mode");
  if (!reach_gap && !reach_radius) return build(nullptr);  // (no records: the plain call)
  GraphReach reach;
  const int rc = graph_reach_of(name, k, reach_gap, reach_radius, nreach, &reach);
  if (rc != G2S_OK) return rc;
  if (mode == G2S_REACH_NEVER) return build(nullptr);
  if (mode == G2S_REACH_AUTO) {
    const int plain = build(nullptr);
    if (plain == G2S_OK || std::string(g2s_last_error()) != kTooManyKmers) return plain;
    if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s] graph build: over the cap, starting over bounded by %llu reach records\n", (unsigned long long)nreach);
  }
  return build(&reach);
}
extern "C" int g2s_graph_build_seqs_reach(const char* const* seqs, const uint64_t* lens, int nseqs, int k, int solid, int nthreads,
                                          const g2s_gap* reach_gap, const int32_t* reach_radius, uint64_t nreach, int mode,
                                          g2s_graph** out) {
  return build_with_reach("g2s_graph_build_seqs_reach", k, reach_gap, reach_radius, nreach, mode, out, [&](const GraphReach* reach) {
    return build_seqs_of(seqs, lens, nseqs, k, solid, nthreads, reach, out);
  });
}
extern "C" int g2s_graph_bounded(const g2s_graph* g) { return g && g->g->bounded ? 1 : 0; }
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_graph_reach(uint64_t* records, uint64_t* seeds, uint64_t* seeds_in_full, uint64_t* full_kmers,
                                         uint64_t* kept_kmers, uint32_t* levels, uint32_t* passes, uint32_t* regrowths, int* on_device,
                                         double* ms_search) {
  const GraphReachInfo info = last_graph_reach();
  if (ms_search) *ms_search = info.ms_search;
  if (records) *records = info.records;
  if (seeds) *seeds = info.seeds;
  if (seeds_in_full) *seeds_in_full = info.seeds_in_full;
  if (full_kmers) *full_kmers = info.full_kmers;
  if (kept_kmers) *kept_kmers = info.kept_kmers;
  if (levels) *levels = info.levels;
  if (passes) *passes = info.passes;
  if (regrowths) *regrowths = info.regrowths;
  if (on_device) *on_device = info.on_device;
  return G2S_OK;
}

extern "C" int g2s_graph_build_sets(const char* const* seqs, const uint64_t* lens, const uint32_t* seq_set, int nseqs,
                                    uint32_t nsets, int k, int solid, int nthreads, g2s_graph** out) {
  if ((!seqs && nseqs) || (!seq_set && nseqs) || !out || nseqs < 0 || nsets == 0) return fail(G2S_ERR_ARG, "g2s_graph_build_sets: bad argument");
  for (int i = 0; i < nseqs; i++)
    if (seq_set[i] >= nsets) return fail(G2S_ERR_ARG, "g2s_graph_build_sets: set id out of range");
  if (nsets == 1) return g2s_graph_build_seqs(seqs, lens, nseqs, k, solid, nthreads, out);  // an ordinary graph
  std::string err;
  Graph* g = graph_build_sets(seq_pairs(seqs, lens, (uint64_t)nseqs), std::vector<uint32_t>(seq_set, seq_set + nseqs), nsets, k, solid,
                              nthreads, &err);
  return wrap_graph(g, err, out);
}
static int build_pool_reach_of(const PoolSets& ps, int k, int solid, int nthreads, const g2s_gap* reach_gap,
                               const int32_t* reach_radius, g2s_graph** out);
// the pooled builds' arguments, checked and as a PoolSets over `v`
static int pool_sets_of(const char* name, const char* const* seqs, const uint64_t* lens, uint64_t nseqs, const uint64_t* set_begin,
                        const uint32_t* set_seq, const uint32_t* shared_seq, uint64_t nshared, const uint8_t* set_shared,
                        uint32_t nsets, g2s_graph** out, std::vector<std::pair<const char*, uint64_t>>* v, PoolSets* ps) {
  if ((!seqs && nseqs && v->size() != nseqs) || !set_begin || !out || nsets == 0 || nseqs >= (1ull << 32) || (!shared_seq && nshared))
    return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
  for (uint32_t s = 0; s < nsets; s++)
    if (set_begin[s + 1] < set_begin[s]) return fail(G2S_ERR_ARG, std::string(name) + ": set_begin decreases");
  if (!set_seq && set_begin[nsets] > set_begin[0]) return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
  // (nullptr with sequences: g2s_graph_build_dpool_reach, which has filled `v` from its pools)
  if (seqs) *v = seq_pairs(seqs, lens, nseqs);
  ps->seqs = v;
  ps->set_begin = set_begin;
  ps->set_seq = set_seq;
  ps->shared_seq = shared_seq;
  ps->nshared = nshared;
  ps->set_shared = set_shared;
  ps->nsets = nsets;
  return G2S_OK;
}
extern "C" int g2s_graph_build_pool(const char* const* seqs, const uint64_t* lens, uint64_t nseqs, const uint64_t* set_begin,
                                    const uint32_t* set_seq, const uint32_t* shared_seq, uint64_t nshared, const uint8_t* set_shared,
                                    uint32_t nsets, int k, int solid, int nthreads, g2s_graph** out) {
  std::vector<std::pair<const char*, uint64_t>> v;
  PoolSets ps;
  const int rc = pool_sets_of("g2s_graph_build_pool", seqs, lens, nseqs, set_begin, set_seq, shared_seq, nshared, set_shared, nsets, out, &v, &ps);
  if (rc != G2S_OK) return rc;
  std::string err;
  return wrap_graph(graph_build_pool(ps, k, solid, nthreads, &err), err, out);
}
extern "C" int g2s_graph_build_pool_reach(const char* const* seqs, const uint64_t* lens, uint64_t nseqs, const uint64_t* set_begin,
                                          const uint32_t* set_seq, const uint32_t* shared_seq, uint64_t nshared,
                                          const uint8_t* set_shared, uint32_t nsets, int k, int solid, int nthreads,
                                          const g2s_gap* reach_gap, const int32_t* reach_radius, g2s_graph** out) {
  if ((reach_gap == nullptr) != (reach_radius == nullptr)) return fail(G2S_ERR_ARG, "g2s_graph_build_pool_reach: reach_gap and reach_radius go together");
  if (!reach_radius) return g2s_graph_build_pool(seqs, lens, nseqs, set_begin, set_seq, shared_seq, nshared, set_shared, nsets, k, solid, nthreads, out);
  std::vector<std::pair<const char*, uint64_t>> v;
  PoolSets ps;
  const int rc = pool_sets_of("g2s_graph_build_pool_reach", seqs, lens, nseqs, set_begin, set_seq, shared_seq, nshared, set_shared, nsets, out, &v, &ps);
  if (rc != G2S_OK) return rc;
  return build_pool_reach_of(ps, k, solid, nthreads, reach_gap, reach_radius, out);
}
// the pooled build with reach records over a checked PoolSets: the host-pointer entry and the device-pool entry alike
static int build_pool_reach_of(const PoolSets& ps, int k, int solid, int nthreads, const g2s_gap* reach_gap,
                               const int32_t* reach_radius, g2s_graph** out) {
  const uint32_t nsets = ps.nsets;
  if (k < 1 || k > kMaxK) return fail(G2S_ERR_ARG, "k must be in [1," + std::to_string(kMaxK) + "]");  // (the seeds below read k characters)
  PoolReach reach;
  reach.radius.assign(reach_radius, reach_radius + nsets);
  reach.seed_begin.assign(1, 0);
  for (uint32_t s = 0; s < nsets; s++) {
    if (reach_radius[s] >= 0) flank_seeds(reach_gap[s], k, &reach.seed);  // (none for the whole set, or a gap the fill rejects)
    reach.seed_begin.push_back(reach.seed.size());
  }
  std::string err;
  return wrap_graph(graph_build_pool_reach(ps, reach, k, solid, nthreads, &err), err, out);
}
// The pooled build over pools the read filter left where it made them (device_pool.h).  A pool held on the build's device
// hands its reads over as null pointers with a PoolDeviceText (dbg_gpu.hip gathers them device to device); every other
// pool hands over host pointers — into its own text when host-held, into a copy that comes down here when it lies on
// another device or the host builds.  The device build giving up later brings the rest down through PoolSets::host_text.
extern "C" int g2s_graph_build_dpool_reach(const g2s_device_pool* const* pools, uint32_t npools, const uint64_t* set_begin,
                                           const uint32_t* set_seq, const uint32_t* shared_seq, uint64_t nshared,
                                           const uint8_t* set_shared, uint32_t nsets, int k, int solid, int nthreads,
                                           const g2s_gap* reach_gap, const int32_t* reach_radius, g2s_graph** out) {
  const char* const name = "g2s_graph_build_dpool_reach";
  if ((reach_gap == nullptr) != (reach_radius == nullptr)) return fail(G2S_ERR_ARG, std::string(name) + ": reach_gap and reach_radius go together");
  if (!pools || npools == 0) return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
  uint64_t total = 0;
  for (uint32_t p = 0; p < npools; p++) {
    if (!pools[p]) return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
    total += pools[p]->view.n_reads;
  }
  if (total >= (1ull << 32)) return fail(G2S_ERR_ARG, std::string(name) + ": bad argument");
  const bool host_build = getenv("G2S_HOST_BUILD") != nullptr;
  const int device = build_device();
  std::vector<std::pair<const char*, uint64_t>> v((size_t)total);
  std::vector<PoolDeviceText> dtext;
  std::vector<std::string> down(npools);  // the text of a device-held pool, once it has come down
  std::vector<uint32_t> first(npools);
  auto point_at = [&](uint32_t p, const char* text) {
    const g2s_device_pool& D = *pools[p];
    for (uint64_t r = 0; r < D.view.n_reads; r++) v[(size_t)(first[p] + r)].first = text + D.start(r);
  };
  auto copy_down = [&](uint32_t p, std::string* err) {
    const g2s_device_pool& D = *pools[p];
    down[p].resize((size_t)D.text_bytes());
    if (!device_pool_copy_down(D.device, D.d_text, 0, D.text_bytes(), &down[p][0], err)) return false;
    point_at(p, down[p].data());
    return true;
  };
  uint64_t at = 0;
  for (uint32_t p = 0; p < npools; p++) {
    const g2s_device_pool& D = *pools[p];
    first[p] = (uint32_t)at;
    for (uint64_t r = 0; r < D.view.n_reads; r++) v[(size_t)(at + r)] = {nullptr, D.base_off[(size_t)r + 1] - D.base_off[(size_t)r]};
    at += D.view.n_reads;
    std::string err;
    if (D.device < 0) point_at(p, D.host_text.data());
    else if (!host_build && D.device == device) dtext.push_back(PoolDeviceText{D.device, (const uint8_t*)D.d_text, D.d_start, first[p], D.view.n_reads});
    else if (!copy_down(p, &err)) return fail(G2S_ERR_HIP, std::string(name) + ": " + err);
  }
  PoolSets ps;
  const int rc = pool_sets_of(name, nullptr, nullptr, total, set_begin, set_seq, shared_seq, nshared, set_shared, nsets, out, &v, &ps);
  if (rc != G2S_OK) return rc;
  if (!dtext.empty()) {
    ps.device_text = &dtext;
    ps.host_text = [&](std::string* err) {
      for (uint32_t p = 0; p < npools; p++)
        if (pools[p]->device >= 0 && down[p].empty() && pools[p]->text_bytes() && !copy_down(p, err)) return false;
      return true;
    };
  }
  if (reach_radius) return build_pool_reach_of(ps, k, solid, nthreads, reach_gap, reach_radius, out);
  std::string err;
  return wrap_graph(graph_build_pool(ps, k, solid, nthreads, &err), err, out);
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_dpool(int* held_on_device, uint64_t* bases_bytes_to_host, uint64_t* text_bytes_gathered_on_device,
                                   uint64_t* text_bytes_packed_on_host) {
  const LastDpoolFilter f = last_dpool_filter();
  const PoolBuildInfo b = last_pool_build();
  if (held_on_device) *held_on_device = f.held_on_device;
  if (bases_bytes_to_host) *bases_bytes_to_host = f.bases_bytes_to_host;
  if (text_bytes_gathered_on_device) *text_bytes_gathered_on_device = b.text_gathered;
  if (text_bytes_packed_on_host) *text_bytes_packed_on_host = b.text_packed;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_pool_reach(uint64_t* reach_sets, uint64_t* full_kmers, int* full_known, uint64_t* kept_kmers,
                                        uint32_t* levels, int* on_device) {
  const PoolReachInfo info = last_pool_reach();
  if (reach_sets) *reach_sets = info.reach_sets;
  if (full_kmers) *full_kmers = info.full_kmers;
  if (full_known) *full_known = info.full_known;
  if (kept_kmers) *kept_kmers = info.kept_kmers;
  if (levels) *levels = info.levels;
  if (on_device) *on_device = info.on_device;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_pool_build(uint64_t* own_positions, uint64_t* shared_positions, uint64_t* keys_sorted, int* on_device) {
  const PoolBuildInfo info = last_pool_build();
  if (own_positions) *own_positions = info.own_positions;
  if (shared_positions) *shared_positions = info.shared_positions;
  if (keys_sorted) *keys_sorted = info.keys_sorted;
  if (on_device) *on_device = info.on_device;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_solid_count(uint64_t* positions, uint32_t* passes, uint32_t* refined_bins, uint64_t* max_pass_keys,
                                         uint64_t* solid, int* on_device) {
  const SolidCountInfo info = last_solid_count();
  if (positions) *positions = info.positions;
  if (passes) *passes = info.passes;
  if (refined_bins) *refined_bins = info.refined_bins;
  if (max_pass_keys) *max_pass_keys = info.max_pass_keys;
  if (solid) *solid = info.solid;
  if (on_device) *on_device = info.on_device;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_plan_passes(const uint64_t* hist, uint32_t nbins, uint64_t cap, uint32_t* first_bin_of_pass,
                                    uint32_t max_passes, uint32_t* npasses, uint32_t* first_oversized_bin) {
  if ((!hist && nbins) || (!first_bin_of_pass && max_passes) || !npasses)
    return fail(G2S_ERR_ARG, "g2s_test_plan_passes: bad argument");
  std::vector<uint32_t> first_bin;
  *npasses = plan_passes(hist, nbins, cap, &first_bin, first_oversized_bin);
  for (uint32_t p = 0; p < std::min(*npasses, max_passes); p++) first_bin_of_pass[p] = first_bin[p];
  return G2S_OK;
}
extern "C" uint32_t g2s_graph_num_sets(const g2s_graph* g) { return g ? g->g->num_sets() : 0; }
extern "C" int g2s_graph_set_nodes(const g2s_graph* g, uint32_t set, uint64_t* first_kmer, uint64_t* n_kmers) {
  if (!g || set >= g->g->num_sets()) return fail(G2S_ERR_ARG, "g2s_graph_set_nodes: bad set");
  const uint64_t lo = g->g->set_lo.empty() ? 0 : g->g->set_lo[set];
  const uint64_t hi = g->g->set_lo.empty() ? g->g->n : g->g->set_lo[(size_t)set + 1];
  if (first_kmer) *first_kmer = lo;
  if (n_kmers) *n_kmers = hi - lo;
  return G2S_OK;
}
extern "C" uint32_t g2s_graph_set_node(const g2s_graph* g, uint32_t set, const char* kmer) {
  if (!g || !kmer || (int)strnlen(kmer, (size_t)g->g->k) < g->g->k) return G2S_INVALID_NODE;
  return g->g->node_of_in(set, kmer);
}

// ---- graphs from read files.  The device loader (reads_text.h) makes the build's text on the device from the files' raw
// bytes and hands it to the device count; the host loader (zlib, parse_fastx, graph_build) is the fallback for everything
// but a file that cannot be read, and what G2S_HOST_BUILD=1, G2S_HOST_READS=1 or a machine without a device get.
namespace {
LastInfo<ReadsLoadInfo> g_reads_info;
void set_reads_info(const ReadsLoadInfo& info) { g_reads_info.set(info); }
uint64_t env_bytes(const char* name) {
  const char* s = getenv(name);
  return s && *s ? strtoull(s, nullptr, 10) : 0;
}
// G2S_BUILD_BAM_STREAM: 1 the BAM read route's streaming form always, 0 never, unset: when resident does not fit
int env_bam_stream() {
  const char* s = getenv("G2S_BUILD_BAM_STREAM");
  return s && *s ? (strcmp(s, "0") != 0 ? 1 : 0) : -1;
}
bool env_on(const char* name) {
  const char* s = getenv(name);
  return s && *s && strcmp(s, "0") != 0;
}
std::vector<std::string> split_csv(const char* reads_csv) {  // comma separated list (Gap2Seq.cpp:199-210)
  std::vector<std::string> files;
  std::string csv(reads_csv);
  size_t pos = 0;
  while (pos <= csv.size()) {
    size_t e = csv.find(',', pos);
    if (e == std::string::npos) e = csv.size();
    if (e > pos) files.push_back(csv.substr(pos, e - pos));
    pos = e + 1;
  }
  return files;
}
}  // namespace

static int build_files_of(const char* reads_csv, int k, int solid, int nthreads, const GraphReach* reach, g2s_graph** out);
extern "C" int g2s_graph_build_files(const char* reads_csv, int k, int solid, int nthreads, g2s_graph** out) {
  return build_files_of(reads_csv, k, solid, nthreads, nullptr, out);
}
extern "C" int g2s_graph_build_files_reach(const char* reads_csv, int k, int solid, int nthreads, const g2s_gap* reach_gap,
                                           const int32_t* reach_radius, uint64_t nreach, int mode, g2s_graph** out) {
  return build_with_reach("g2s_graph_build_files_reach", k, reach_gap, reach_radius, nreach, mode, out, [&](const GraphReach* reach) {
    return build_files_of(reads_csv, k, solid, nthreads, reach, out);
  });
}
static int build_files_of(const char* reads_csv, int k, int solid, int nthreads, const GraphReach* reach, g2s_graph** out) {
  if (!reads_csv || !out) return fail(G2S_ERR_ARG, "g2s_graph_build_files: bad argument");
  const std::vector<std::string> files = split_csv(reads_csv);
  const bool debug = getenv("G2S_DEBUG") != nullptr;
  int bam_reason = kBamReadsNotAsked, bam_anomaly = 0;  // what the device loader met in a BAM file, when it gave up
  // (G2S_HOST_BUILD: set to anything, as graph_build reads it)
  if (!getenv("G2S_HOST_BUILD") && !env_on("G2S_HOST_READS")) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<ReadsInput> inputs(files.size());
    for (size_t i = 0; i < files.size(); i++) inputs[i].path = files[i];
    const uint64_t piece = env_bytes("G2S_BUILD_PIECE_BYTES");
    DeviceText text;
    ReadsLoadInfo info;
    std::string why;
    const ReadsLoadResult r = load_reads_device(inputs, build_device(), (size_t)piece, env_bytes("G2S_BUILD_TEXT_FIRST_BYTES"),
                                                env_on("G2S_HOST_INFLATE"), &text, &info, &why, env_bytes("G2S_BUILD_RESIDENT_CAP"),
                                                env_bam_stream(), device_gzip_asked());
    if (r == kReadsIoError) return fail(G2S_ERR_IO, why);
    if (r != kReadsOk) { bam_reason = info.bam_reason; bam_anomaly = info.bam_anomaly; }
    if (r == kReadsOk && text.T == 0) {  // (no sequence at all: the empty graph, as the host loader builds it)
      free_device_text(&text);
      why = "no text";
    } else if (r == kReadsOk) {
      if (debug)
        fprintf(stderr, "[g2s] reads: %llu files, %llu raw bytes, %llu text positions, %llu records in %llu pieces on the device, %.3f s\n",
                (unsigned long long)info.files, (unsigned long long)info.raw_bytes, (unsigned long long)info.positions,
                (unsigned long long)info.records, (unsigned long long)info.pieces, ms_since(t0) / 1e3);
      bool gave_up = false;
      std::string err;
      Graph* g = graph_build_text(&text, k, solid, nthreads, &err, &gave_up, reach);
      free_device_text(&text);
      if (g) set_reads_info(info);
      if (g || !gave_up) return wrap_graph(g, err, out);
      why = "the device count gave up: " + err;
    }
    if (debug) fprintf(stderr, "[g2s] reads: the host loader takes over (%s)\n", why.c_str());
  }
  ReadsLoadInfo info;
  info.bam_reason = bam_reason;
  info.bam_anomaly = bam_anomaly;
  std::vector<FastxRecord> recs;
  for (const std::string& file : files) {
    std::string raw, text, err;
    if (!read_text_file(file, &raw)) return fail(G2S_ERR_IO, "cannot read " + file);
    const uint8_t* bytes = (const uint8_t*)raw.data();
    const bool gz = is_gzip(bytes, raw.size());
    info.files++;
    info.inflate.push_back(gz ? kInflateZlib : kInflateNone);
    if (gz && is_bam(bytes, raw.size())) {  // (bam_reads.h: the kept records' sequences, by the reader's walk)
      ReadsInput in;
      in.path = file;
      in.mem = bytes;
      in.mem_n = raw.size();
      std::vector<std::string> seqs;
      if (!bam_reads_host(in, &seqs, &info.bam_skipped, &info.raw_bytes, &err)) return fail(G2S_ERR_IO, err);
      info.bam_files++;
      info.bam_kept += seqs.size();
      for (std::string& q : seqs) {
        recs.emplace_back();
        recs.back().seq.swap(q);
      }
      continue;
    }
    if (!gz) text.swap(raw);
    else if (!reads_text_of_bytes(bytes, raw.size(), file, &text, nullptr, &err)) return fail(G2S_ERR_IO, err);
    info.raw_bytes += text.size();
    parse_fastx(text, &recs);
  }
  std::vector<std::pair<const char*, uint64_t>> v;
  for (auto& r : recs) {
    v.emplace_back(r.seq.data(), (uint64_t)r.seq.size());
    info.positions += r.seq.size() + 1;
  }
  info.records = recs.size();
  std::string err;
  Graph* g = graph_build(v, k, solid, nthreads, &err, reach);
  if (g) set_reads_info(info);
  return wrap_graph(g, err, out);
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_reads_load(uint64_t* files, uint64_t* raw_bytes, uint64_t* positions, uint64_t* records,
                                        uint64_t* pieces, int* on_device, int* inflate, uint64_t inflate_cap, uint64_t* grows) {
  const ReadsLoadInfo info = g_reads_info.get();
  if (files) *files = info.files;
  if (raw_bytes) *raw_bytes = info.raw_bytes;
  if (positions) *positions = info.positions;
  if (records) *records = info.records;
  if (pieces) *pieces = info.pieces;
  if (on_device) *on_device = info.on_device;
  if (grows) *grows = info.grows;
  if (inflate)
    for (uint64_t i = 0; i < std::min<uint64_t>(inflate_cap, info.inflate.size()); i++) inflate[i] = info.inflate[i];
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_reads_bam(uint64_t* bam_files, uint64_t* kept, uint64_t* skipped, int* by_kernels, int* reason,
                                       int* anomaly) {
  const ReadsLoadInfo info = g_reads_info.get();
  if (bam_files) *bam_files = info.bam_files;
  if (kept) *kept = info.bam_kept;
  if (skipped) *skipped = info.bam_skipped;
  if (by_kernels) *by_kernels = info.bam_kernels;
  if (reason) *reason = info.bam_reason;
  if (anomaly) *anomaly = info.bam_anomaly;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_reads_bam_stream(uint64_t* streamed_files, uint64_t* windows, uint64_t* peak_device_bytes) {
  const ReadsLoadInfo info = g_reads_info.get();
  if (streamed_files) *streamed_files = info.bam_streamed;
  if (windows) *windows = info.bam_stream_windows;
  if (peak_device_bytes) *peak_device_bytes = info.bam_stream_peak;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_reads_text(const void* bytes, size_t n, int device, size_t piece_bytes, uint8_t* out, size_t cap,
                                   size_t* out_n) {
  if ((!bytes && n) || (!out && cap) || !out_n || device < -2) return fail(G2S_ERR_ARG, "g2s_test_reads_text: bad argument");
  const uint8_t* p = (const uint8_t*)bytes;
  if (device < 0) {
    std::string raw, err, text;
    ReadsLoadInfo info;
    info.files = 1;
    if (is_bam(p, n)) {  // (either host form: there is no line machine for BAM)
      ReadsInput in;
      in.mem = p;
      in.mem_n = n;
      std::vector<std::string> seqs;
      if (!bam_reads_host(in, &seqs, &info.bam_skipped, &info.raw_bytes, &err)) return fail(G2S_ERR_IO, err);
      for (const std::string& q : seqs) { text += q; text.push_back('N'); }
      info.records = info.bam_kept = seqs.size();
      info.bam_files = 1;
      info.inflate.push_back(kInflateZlib);
    } else {
      if (!reads_text_of_bytes(p, n, "(memory)", &raw, nullptr, &err)) return fail(G2S_ERR_IO, err);
      info.raw_bytes = raw.size();
      if (device == -1) {
        std::vector<FastxRecord> recs;
        parse_fastx(raw, &recs);
        for (auto& r : recs) { text += r.seq; text.push_back('N'); }
        info.records = recs.size();
      } else {
        machine_text_host((const uint8_t*)raw.data(), raw.size(), &text, &info.records);
      }
    }
    info.positions = text.size();
    set_reads_info(info);
    *out_n = text.size();
    if (!text.empty()) memcpy(out, text.data(), std::min(cap, text.size()));
    return G2S_OK;
  }
  if (!filter_device_usable(device)) return fail(G2S_ERR_NO_DEVICE, "g2s_test_reads_text: no usable gfx950 device " + std::to_string(device));
  std::vector<ReadsInput> inputs(1);
  inputs[0].mem = p;
  inputs[0].mem_n = n;
  DeviceText text;
  ReadsLoadInfo info;
  std::string why;
  const ReadsLoadResult r = load_reads_device(inputs, device, piece_bytes,
                                              env_bytes("G2S_BUILD_TEXT_FIRST_BYTES"), env_on("G2S_HOST_INFLATE"), &text, &info, &why,
                                              env_bytes("G2S_BUILD_RESIDENT_CAP"), env_bam_stream(), device_gzip_asked());
  if (r == kReadsIoError) return fail(G2S_ERR_IO, why);
  if (r != kReadsOk) {
    info.bam_streamed = info.bam_stream_windows = info.bam_stream_peak = 0;  // (nothing of a refused call counts)
    set_reads_info(info);  // (g2s_test_last_reads_bam: what a BAM file met)
    return fail(G2S_ERR_HIP, "g2s_test_reads_text: the device refused (" + why + ")");
  }
  set_reads_info(info);
  *out_n = (size_t)text.T;
  const size_t take = std::min<size_t>(cap, (size_t)text.T);
  const hipError_t e = take ? hipMemcpy(out, text.d_text, take, hipMemcpyDeviceToHost) : hipSuccess;
  free_device_text(&text);
  if (e != hipSuccess) return fail(G2S_ERR_HIP, std::string("g2s_test_reads_text: ") + hipGetErrorString(e));
  return G2S_OK;
}

extern "C" int g2s_reads_set_device_gzip(int mode) { return set_device_gzip(mode); }
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_last_reads_gzip(uint64_t* files, uint64_t* windows, uint64_t* chunks, uint64_t* starts_found,
                                        uint64_t* absorbed, uint64_t* members, int* outcome, uint64_t* peak_device_bytes) {
  const ReadsLoadInfo info = g_reads_info.get();
  if (files) *files = info.gzip.files;
  if (windows) *windows = info.gzip.windows;
  if (chunks) *chunks = info.gzip.chunks;
  if (starts_found) *starts_found = info.gzip.starts_found;
  if (absorbed) *absorbed = info.gzip.absorbed;
  if (members) *members = info.gzip.members;
  if (outcome) *outcome = info.gzip.outcome;
  if (peak_device_bytes) *peak_device_bytes = info.gzip.peak_device_bytes;
  return G2S_OK;
}
// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_gzip_inflate(const void* bytes, size_t n, int device, uint32_t chunk_bytes, uint32_t window_chunks,
                                     uint8_t* out, size_t cap, size_t* out_n, int* outcome) {
  if (!bytes || !out_n || (!out && cap) || device < -2) return fail(G2S_ERR_ARG, "g2s_test_gzip_inflate: bad argument");
  *out_n = 0;
  if (outcome) *outcome = kGzDone;
  const uint8_t* p = (const uint8_t*)bytes;
  std::string all;
  if (device == -1) {
    std::string err;
    if (!reads_text_of_bytes(p, n, "(memory)", &all, nullptr, &err)) return fail(G2S_ERR_IO, err);
  } else {
    GzipParams P = gzip_params_from_env();
    if (chunk_bytes) P.chunk = std::max<uint32_t>(chunk_bytes, 1024);
    // (0: the whole file in one window)
    P.window_chunks = window_chunks ? std::max<uint32_t>(window_chunks, 2) : (uint32_t)std::min<uint64_t>(65535, std::max<uint64_t>(n / P.chunk + 1, 2));
    std::unique_ptr<GzipBackend> B;
    if (device >= 0) {
      if (!filter_device_usable(device)) return fail(G2S_ERR_NO_DEVICE, "g2s_test_gzip_inflate: no usable gfx950 device " + std::to_string(device));
      std::string why;
      if (hipSetDevice(device) != hipSuccess) return fail(G2S_ERR_HIP, "g2s_test_gzip_inflate: the device cannot be used");
      B = make_gzip_device_backend(device, nullptr, P, &why);
      if (!B) return fail(G2S_ERR_HIP, "g2s_test_gzip_inflate: " + why);
    } else {
      B = make_gzip_host_backend(P);
    }
    GzipStats st;
    std::string hip_why;
    const int oc = gzip_route(
        p, n, P, *B, &st, []() -> uint32_t { return 0; },
        [&](const uint8_t* from, uint64_t m, bool) -> bool {
          if (!m) return true;
          const size_t at = all.size();
          all.resize(at + m);
          if (device < 0) {
            memcpy(&all[at], from, m);
            return true;
          }
          const hipError_t e = hipMemcpy(&all[at], from, m, hipMemcpyDeviceToHost);
          if (e != hipSuccess) hip_why = hipGetErrorString(e);
          return e == hipSuccess;
        });
    ReadsLoadInfo info;
    info.gzip = st;
    info.gzip.peak_device_bytes = B->device_bytes();
    set_reads_info(info);
    if (oc == kGzHip) return fail(G2S_ERR_HIP, "g2s_test_gzip_inflate: " + (hip_why.empty() ? B->why : hip_why));
    if (outcome) *outcome = oc;
    if (oc != kGzDone) return G2S_OK;  // (given back: no bytes)
  }
  *out_n = all.size();
  if (!all.empty()) memcpy(out, all.data(), std::min(cap, all.size()));
  return G2S_OK;
}

extern "C" int g2s_graph_save(const g2s_graph* g, const char* path) {
  std::string err;
  if (!g || !path) return fail(G2S_ERR_ARG, "g2s_graph_save: bad argument");
  if (g->g->num_sets() > 1) return fail(G2S_ERR_ARG, "g2s_graph_save: graphs of several read sets are not saved");
  return graph_save(*g->g, path, &err) ? G2S_OK : fail(G2S_ERR_IO, err);
}
extern "C" int g2s_graph_load(const char* path, g2s_graph** out) {
  std::string err;
  if (!path || !out) return fail(G2S_ERR_ARG, "g2s_graph_load: bad argument");
  Graph* g = graph_load(path, &err);
  if (!g) return fail(G2S_ERR_IO, err);
  *out = new g2s_graph();
  (*out)->g = g;
  return G2S_OK;
}
extern "C" void g2s_graph_free(g2s_graph* g) {
  if (!g) return;
  if (g->g) {
    for (auto& kv : g->g->dev) {
      if (hipSetDevice(kv.first) == hipSuccess) {
        if (kv.second.succ) (void)hipFree(kv.second.succ);
        if (kv.second.pred) (void)hipFree(kv.second.pred);
        if (kv.second.ustart) (void)hipFree(kv.second.ustart - kUstartPad);
        if (kv.second.rem) (void)hipFree(kv.second.rem);
        if (kv.second.urec) (void)hipFree(kv.second.urec);
        if (kv.second.brec) (void)hipFree(kv.second.brec);
      }
    }
    delete g->g;
  }
  delete g;
}
extern "C" int g2s_graph_k(const g2s_graph* g) { return g ? g->g->k : 0; }
extern "C" int g2s_graph_solid(const g2s_graph* g) { return g ? g->g->solid : 0; }
extern "C" uint64_t g2s_graph_num_kmers(const g2s_graph* g) { return g ? g->g->n : 0; }
extern "C" uint64_t g2s_graph_num_unitigs(const g2s_graph* g) { return g ? g->g->n_unitigs : 0; }
extern "C" uint32_t g2s_graph_node(const g2s_graph* g, const char* kmer) {
  if (!g || !kmer || (int)strnlen(kmer, (size_t)g->g->k) < g->g->k) return G2S_INVALID_NODE;
  return g->g->node_of(kmer);
}
extern "C" int g2s_graph_successors(const g2s_graph* g, uint32_t node, uint32_t out[4]) {
  if (!g || (uint64_t)node >= 2 * g->g->n) return 0;
  int c = 0;
  for (int nt = 0; nt < 4; nt++) {
    uint32_t w = g->g->succ_of(node, nt);
    if (w != kInvalidNode) out[c++] = w;
  }
  return c;
}
extern "C" int g2s_graph_predecessors(const g2s_graph* g, uint32_t node, uint32_t out[4]) {
  if (!g || (uint64_t)node >= 2 * g->g->n) return 0;
  int c = 0;
  for (int nt = 0; nt < 4; nt++) {
    uint32_t w = g->g->pred_of(node, nt);
    if (w != kInvalidNode) out[c++] = w;
  }
  return c;
}
extern "C" int g2s_graph_node_string(const g2s_graph* g, uint32_t node, char* out) {
  if (!g || !out || (uint64_t)node >= 2 * g->g->n) return fail(G2S_ERR_ARG, "g2s_graph_node_string: bad node");
  std::string s = g->g->node_string(node);
  memcpy(out, s.c_str(), s.size() + 1);
  return G2S_OK;
}

extern "C" int g2s_graph_upload(g2s_graph* gh, int device) {
  g2s_env_sync();
  if (!gh) return fail(G2S_ERR_ARG, "g2s_graph_upload: null graph");
  Graph& g = *gh->g;
  if (g.dev.count(device)) return G2S_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(G2S_ERR_NO_DEVICE, "no HIP device " + std::to_string(device) + " (this library has no CPU fallback)");
  HIP_TRY(hipSetDevice(device));
  DeviceGraph dg;
  const size_t bytes = g.succ.size() * sizeof(uint32_t);
  // 1 KB of INVALID entries behind the table: a read a little past its last row finds no successor
  HIP_TRY(hipMalloc((void**)&dg.succ, bytes + 1024));
  HIP_TRY(hipMemset(dg.succ, 0xFF, bytes + 1024));
  HIP_TRY(hipMemcpy(dg.succ, g.succ.data(), bytes, hipMemcpyHostToDevice));
  dg.bytes = bytes;
  if (!g.pred.empty()) {
    HIP_TRY(hipMalloc((void**)&dg.pred, bytes));
    HIP_TRY(hipMemcpy(dg.pred, g.pred.data(), bytes, hipMemcpyHostToDevice));
    dg.bytes += bytes;
  }
  {  // unitig-start bitmap between two pads of all-ones words (scans past either end stop there)
    const size_t words = g.ustart.size();
    uint64_t* base = nullptr;
    HIP_TRY(hipMalloc((void**)&base, (words + 2 * kUstartPad) * 8));
    HIP_TRY(hipMemset(base, 0xFF, (words + 2 * kUstartPad) * 8));
    HIP_TRY(hipMemcpy(base + kUstartPad, g.ustart.data(), words * 8, hipMemcpyHostToDevice));
    dg.ustart = base + kUstartPad;
    dg.bytes += (words + 2 * kUstartPad) * 8;
  }
  g.dev[device] = dg;
  return G2S_OK;
}
extern "C" uint64_t g2s_graph_device_bytes(const g2s_graph* g, int device) {
  if (!g) return 0;
  auto it = g->g->dev.find(device);
  return it == g->g->dev.end() ? 0 : it->second.bytes;
}

extern "C" int64_t g2s_graph_validate(const g2s_graph* gr, char* msg, size_t msg_cap) {
  if (!gr || !gr->g) return -1;
  const Graph& g = *gr->g;
  std::string text;
  int64_t bad = 0;
  auto note = [&](const char* what, uint64_t i) {
    if (bad++ < 8) text += std::string(what) + " at k-mer " + std::to_string(i) + "; ";
  };
  auto only = [&](uint32_t v, uint32_t want) {  // the single valid successor of v is `want`
    int cnt = 0;
    bool hit = false;
    for (int nt = 0; nt < 4; nt++) {
      const uint32_t w = g.succ_of(v, nt);
      if (w == kInvalidNode) continue;
      cnt++;
      hit = hit || w == want;
    }
    return cnt == 1 && hit;
  };
  uint64_t starts = 0;
  for (uint64_t i = 0; i < g.n; i++) {
    const bool start = (g.ustart[i >> 6] >> (i & 63)) & 1;
    starts += start;
    if (i == 0) { if (!start) note("first k-mer is not a unitig start", i); continue; }
    if (start) continue;
    const uint32_t a = (uint32_t)(2 * (i - 1)), b = (uint32_t)(2 * i);
    if (!only(a, b)) note("internal edge is not the only successor (even orientation)", i);
    if (!only(b ^ 1u, a ^ 1u)) note("internal edge is not the only successor (odd orientation)", i);
  }
  if (starts != g.n_unitigs) note("bitmap population differs from the unitig count", starts);
  if (!g.set_lo.empty()) {  // set graphs: the sets' ranges tile the nodes, no edge leaves its set
    if (g.set_lo.front() != 0 || g.set_lo.back() != g.n) note("set ranges do not cover the k-mers", g.n);
    for (size_t s = 0; s + 1 < g.set_lo.size(); s++) {
      if (g.set_lo[s] > g.set_lo[s + 1]) { note("set ranges not ascending", g.set_lo[s]); continue; }
      for (uint64_t i = g.set_lo[s]; i < g.set_lo[s + 1]; i++)
        for (uint32_t v = (uint32_t)(2 * i); v <= (uint32_t)(2 * i + 1); v++)
          for (int nt = 0; nt < 4; nt++) {
            const uint32_t w = g.succ_of(v, nt);
            if (w != kInvalidNode && ((w >> 1) < g.set_lo[s] || (w >> 1) >= g.set_lo[s + 1])) note("successor outside its set", i);
          }
    }
  }
  for (uint64_t v = 0; v < 2 * g.n; v++)
    for (int nt = 0; nt < 4; nt++) {
      const uint32_t w = g.succ_of((uint32_t)v, nt);
      if (w == kInvalidNode) continue;
      if (w >= 2 * g.n) { note("successor out of range", v >> 1); continue; }
      if (g.lastnt[w] != nt) note("last base of a successor differs from its slot", v >> 1);
    }
  if (msg && msg_cap) {
    const size_t c = std::min(text.size(), msg_cap - 1);
    memcpy(msg, text.data(), c);
    msg[c] = 0;
  }
  return bad;
}
