// gap2seq_amd/csrc/graph_reach.h — a single graph bounded to what its gap list can reach (dbg.hpp: GraphReach), on the
// device.  A device header of dbg_gpu.hip (included once, at file scope, behind its kernels: it uses d_revcomp, DevMem and
// the scan helpers as they are).
//
// The solid table — the sorted canonical k-mers of the whole read set — stays in device memory and may hold any number
// of keys the device has room for: every index into it is 64 bits wide, the prefix index (k_bucket64) included.  What
// leaves is the KEPT set, which is an ordinary set below the graph's cap.
//
// One level-synchronous search serves all records.  With Rmax the largest radius, a record's seeds enter at level
// Rmax - radius; one bit a solid k-mer marks what is visited; a k-mer is claimed (atomicOr on its bit) at the earliest
// level that reaches it, which is the one that leaves it the most budget, so what is visited after level Rmax is the
// union of the records' balls.  Claimed indices are appended to ONE queue — votes and prefix counts in a wave, one add on
// the tail a wave — and level L's frontier is the slice [lo, hi) of that queue; at the end the queue holds every kept
// index once.  A level is at most three launches: k_reach_seeds (only when seeds enter), k_reach_close (one thread: lo =
// hi, hi = tail) and k_reach_expand, which takes its frontier bounds from device memory.  No workgroup waits for
// another.  The host reads the control words back every REACH_SYNC_LEVELS levels: to stop when nothing is left to
// expand and no seed is to come, to jump to the next level at which seeds enter, or — the queue having overflowed — to
// run the search again with a larger queue.  Nothing is written at or beyond the queue's capacity.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdlib>

namespace {

constexpr int REACH_THREADS = 256;
constexpr unsigned REACH_GRID = 1024;
constexpr uint32_t REACH_SYNC_LEVELS = 8;

struct ReachCtl {
  unsigned long long tail;      // entries appended (beyond cap: counted, not written)
  unsigned long long lo, hi;    // the frontier of the level being expanded
  unsigned long long overflow;  // an append found no room
  unsigned long long seeds_in;  // seeds that are solid k-mers (counted with their copies)
};

// bucket[b] = first index whose top bits are >= b, b in [0, nb]
template <class KT>
__global__ void k_bucket64(const KT* __restrict__ v, uint64_t n, int shift, uint32_t nb, uint64_t* __restrict__ bucket) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)(v[mid] >> shift) < (uint64_t)b) lo = mid + 1; else hi = mid;
  }
  bucket[b] = lo;
}

constexpr uint64_t REACH_NONE = ~0ull;

template <class KT>
__device__ __forceinline__ uint64_t d_find64(const KT* __restrict__ v, const uint64_t* __restrict__ bucket, int shift, const KT& x) {
  const uint64_t b = (uint64_t)(x >> shift);
  uint64_t lo = bucket[b], hi = bucket[b + 1];
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < end && v[lo] == x) ? lo : REACH_NONE;
}

// true for the one lane that sets the bit of index i
__device__ __forceinline__ bool d_reach_claim(uint32_t* __restrict__ vis, uint64_t i) {
  const uint32_t bit = 1u << (uint32_t)(i & 31u);
  return !(atomicOr(&vis[i >> 5], bit) & bit);
}

// Every lane of the wave comes here together.  The claimed indices go behind the queue's tail: one add a wave.
__device__ __forceinline__ void d_reach_append(bool claimed, uint64_t idx, uint64_t* __restrict__ queue, uint64_t cap, ReachCtl* ctl) {
  const uint64_t votes = __ballot(claimed);
  if (votes == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long at = 0;
  if (lane == 0) at = atomicAdd(&ctl->tail, (unsigned long long)__popcll(votes));
  at = __shfl(at, 0);
  const uint64_t to = at + (uint64_t)__popcll(votes & ((1ull << lane) - 1ull));
  if (claimed) {
    if (to < cap) queue[to] = idx;
    else ctl->overflow = 1ull;
  }
}

// the seeds [s0, s1) that are solid k-mers and not yet visited are claimed and appended
template <class KT>
__global__ __launch_bounds__(REACH_THREADS) void k_reach_seeds(const KT* __restrict__ table, const uint64_t* __restrict__ bucket, int shift,
                                                               const KT* __restrict__ seeds, uint64_t s0, uint64_t s1,
                                                               uint32_t* __restrict__ vis, uint64_t* __restrict__ queue, uint64_t cap,
                                                               ReachCtl* ctl) {
  const uint64_t total = s1 - s0, stride = (uint64_t)gridDim.x * REACH_THREADS;
  for (uint64_t base = (uint64_t)blockIdx.x * REACH_THREADS; base < total; base += stride) {  // (the same trips in every lane)
    const uint64_t i = base + threadIdx.x;
    uint64_t idx = REACH_NONE;
    if (i < total) idx = d_find64<KT>(table, bucket, shift, seeds[s0 + i]);
    const uint64_t found = __ballot(idx != REACH_NONE);
    if (found && (threadIdx.x & 63u) == 0) atomicAdd(&ctl->seeds_in, (unsigned long long)__popcll(found));
    const bool claimed = idx != REACH_NONE && d_reach_claim(vis, idx);
    d_reach_append(claimed, idx, queue, cap, ctl);
  }
}

// the level's frontier is what the queue gained since the last one's
__global__ void k_reach_close(ReachCtl* ctl, uint64_t cap) {
  if (blockIdx.x || threadIdx.x) return;
  ctl->lo = ctl->hi;
  ctl->hi = ctl->tail < cap ? ctl->tail : cap;
}

// lane = (frontier k-mer, neighbour): the eight neighbours of queue[lo .. hi) that are solid and not yet visited are
// claimed and appended (behind hi: they are the next level's frontier)
template <class KT>
__global__ __launch_bounds__(REACH_THREADS) void k_reach_expand(const KT* __restrict__ table, const uint64_t* __restrict__ bucket, int shift,
                                                                int k, uint32_t* __restrict__ vis, uint64_t* __restrict__ queue, uint64_t cap,
                                                                ReachCtl* ctl) {
  const uint64_t lo = ctl->lo, hi = ctl->hi;  // (written by k_reach_close, the launch before; nothing writes them now)
  const uint64_t total = (hi - lo) * 8ull, stride = (uint64_t)gridDim.x * REACH_THREADS;
  const KT mask = (2 * k >= (int)(8 * sizeof(KT))) ? ~(KT)0 : ((((KT)1) << (2 * k)) - 1);
  for (uint64_t base = (uint64_t)blockIdx.x * REACH_THREADS; base < total; base += stride) {
    const uint64_t item = base + threadIdx.x;
    uint64_t idx = REACH_NONE;
    if (item < total) {
      const KT c = table[queue[lo + (item >> 3)]], rc = d_revcomp(c, k);
      const uint32_t nb = (uint32_t)(item & 7u), nt = nb & 3u;
      const KT seq = (nb & 4u) ? rc : c, rseq = (nb & 4u) ? c : rc;
      const KT y = ((seq << 2) | (KT)(uint64_t)nt) & mask;
      const KT ry = (rseq >> 2) | ((KT)(uint64_t)(nt ^ 2u) << (2 * (k - 1)));
      idx = d_find64<KT>(table, bucket, shift, y < ry ? y : ry);
    }
    const bool claimed = idx != REACH_NONE && d_reach_claim(vis, idx);
    d_reach_append(claimed, idx, queue, cap, ctl);
  }
}

// the kept keys in table order: a thread a word of the bitmap
__global__ void k_reach_word_count(const uint32_t* __restrict__ vis, uint64_t nwords, uint64_t* __restrict__ cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < nwords) cnt[w] = (uint64_t)__popc(vis[w]);
}
template <class KT>
__global__ void k_reach_compact(const KT* __restrict__ table, const uint32_t* __restrict__ vis, const uint64_t* __restrict__ pos,
                                uint64_t nwords, uint64_t nkept, KT* __restrict__ out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  uint32_t bits = vis[w];
  uint64_t to = pos[w];
  while (bits) {
    const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
    bits &= bits - 1u;
    if (to < nkept) out[to] = table[w * 32ull + b];  // (the bitmap has no bit at or beyond the table's end)
    to++;
  }
}

}  // namespace

namespace g2s {

void set_graph_reach_info(const GraphReachInfo& info);  // dbg.cpp

static uint64_t reach_env_u64(const char* name) {
  const char* s = getenv(name);
  return s && *s ? strtoull(s, nullptr, 10) : 0;
}

// The kept set of the sorted solid table d_table[0 .. n) (n > 0) for the records of `reach`: d_kept[0 .. *nkept), sorted.
// When *nkept reaches the graph's cap nothing is compacted (d_kept stays empty): the build refuses such a set.  false with
// a reason when the device cannot take it (an allocation, a HIP error): the host path builds the same graph.
template <class KT>
static bool reach_on_device(const KT* d_table, uint64_t n, int k, const GraphReach& reach, DevMem& d_kept, uint64_t* nkept,
                            std::string* why, GraphReachInfo* info) {
  const ReachSeeds<KT> rs = make_reach_seeds<KT>(reach, k);
  info->records = reach.records;
  info->seeds = reach.seed.size();
  info->full_kmers = n;
  info->on_device = 1;
  *nkept = 0;
  if (rs.key.empty()) return true;
  int bits = 22;
  while (bits < 28 && (1ull << (bits + 3)) < n) bits++;
  bits = std::min(2 * k, bits);
  const int shift = 2 * k - bits;
  const uint32_t nb = 1u << bits;
  const uint64_t nwords = (n + 31) / 32;
  DevMem d_bucket, d_seeds, d_vis, d_ctl, d_queue;
  G2S_HIP_TRY(d_bucket.alloc(((size_t)nb + 1) * 8));
  G2S_HIP_TRY(d_seeds.alloc(rs.key.size() * sizeof(KT)));
  G2S_HIP_TRY(d_vis.alloc((size_t)nwords * 4));
  G2S_HIP_TRY(d_ctl.alloc(sizeof(ReachCtl)));
  const dim3 blk(REACH_THREADS);
  hipLaunchKernelGGL(k_bucket64<KT>, dim3((nb + 1 + 255) / 256), dim3(256), 0, 0, d_table, n, shift, nb, d_bucket.as<uint64_t>());
  G2S_HIP_TRY(hipGetLastError());
  G2S_HIP_TRY(hipMemcpy(d_seeds.p, rs.key.data(), rs.key.size() * sizeof(KT), hipMemcpyHostToDevice));
  // the queue: every kept index once, so n entries always suffice; it starts smaller and grows on overflow
  const uint64_t asked = reach_env_u64("G2S_REACH_QUEUE_CAP");
  uint64_t cap = std::min<uint64_t>(n, asked ? asked : (1ull << 22));
  ReachCtl ctl;
  uint32_t level = 0;
  auto t_search = std::chrono::steady_clock::now();
  while (true) {
    d_queue.free();
    G2S_HIP_TRY(d_queue.alloc((size_t)cap * 8));
    G2S_HIP_TRY(hipMemset(d_vis.p, 0, (size_t)nwords * 4));
    G2S_HIP_TRY(hipMemset(d_ctl.p, 0, sizeof(ReachCtl)));
    bool done = false;
    uint32_t since_sync = 0;
    t_search = std::chrono::steady_clock::now();
    level = 0;
    size_t cursor = 0;
    while (!done) {
      uint64_t s0, s1;
      rs.at(level, &cursor, &s0, &s1);
      if (s1 > s0)
        hipLaunchKernelGGL(k_reach_seeds<KT>, dim3((unsigned)std::min<uint64_t>((s1 - s0 + REACH_THREADS - 1) / REACH_THREADS, REACH_GRID)), blk,
                           0, 0, d_table, (const uint64_t*)d_bucket.p, shift, (const KT*)d_seeds.p, s0, s1, d_vis.as<uint32_t>(),
                           d_queue.as<uint64_t>(), cap, (ReachCtl*)d_ctl.p);
      hipLaunchKernelGGL(k_reach_close, dim3(1), dim3(64), 0, 0, (ReachCtl*)d_ctl.p, cap);
      if (level < rs.rmax)
        hipLaunchKernelGGL(k_reach_expand<KT>, dim3(REACH_GRID), blk, 0, 0, d_table, (const uint64_t*)d_bucket.p, shift, k,
                           d_vis.as<uint32_t>(), d_queue.as<uint64_t>(), cap, (ReachCtl*)d_ctl.p);
      G2S_HIP_TRY(hipGetLastError());
      if (level == rs.rmax || ++since_sync >= REACH_SYNC_LEVELS) {
        since_sync = 0;
        G2S_HIP_TRY(hipMemcpy(&ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl.overflow || level == rs.rmax) break;
        if (ctl.tail == ctl.hi) {  // this level claimed nothing: the next frontier is what enters
          if (cursor == rs.entry.size()) break;
          level = rs.entry[cursor];
          continue;
        }
      }
      level++;
    }
    if (!ctl.overflow) break;
    if (cap >= n) { if (why) *why = "the reach queue overflowed at the table's size"; return false; }
    cap = std::min<uint64_t>(n, cap * 4);
    info->regrowths++;
  }
  info->ms_search = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_search).count();
  info->levels = level;  // (where the loop stopped: up to REACH_SYNC_LEVELS - 1 behind the last level that claimed a k-mer)
  info->seeds_in_full = ctl.seeds_in;
  info->kept_kmers = *nkept = ctl.tail;
  if (*nkept == 0 || *nkept >= graph_max_kmers()) return true;
  d_queue.free();
  DevMem d_cnt, d_pos;
  G2S_HIP_TRY(d_cnt.alloc((size_t)nwords * 8));
  G2S_HIP_TRY(d_pos.alloc((size_t)nwords * 8));
  G2S_HIP_TRY(d_kept.alloc((size_t)*nkept * sizeof(KT)));
  const dim3 grdW((unsigned)((nwords + 255) / 256));
  hipLaunchKernelGGL(k_reach_word_count, grdW, dim3(256), 0, 0, (const uint32_t*)d_vis.p, nwords, d_cnt.as<uint64_t>());
  uint64_t total = 0;
  G2S_HIP_TRY(scan_total((const uint64_t*)d_cnt.p, d_pos.as<uint64_t>(), (size_t)nwords, &total));
  if (total != *nkept) { if (why) *why = "the reach bitmap holds " + std::to_string(total) + " k-mers, the queue " + std::to_string(*nkept); return false; }
  hipLaunchKernelGGL(k_reach_compact<KT>, grdW, dim3(256), 0, 0, d_table, (const uint32_t*)d_vis.p, (const uint64_t*)d_pos.p, nwords, *nkept,
                     d_kept.as<KT>());
  G2S_HIP_TRY(hipGetLastError());
  G2S_HIP_TRY(hipDeviceSynchronize());
  return true;
}

}  // namespace g2s
