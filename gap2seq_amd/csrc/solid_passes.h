// gap2seq_amd/csrc/solid_passes.h — the solid k-mer set of one graph in key-range passes, for read sets beyond one sort.
// A device header of dbg_gpu.hip (included once, at file scope, behind its kernels and sort helpers): it uses d_revcomp's
// neighbours k_heads / k_head_index / k_solid_flag / k_compact and sort_keyed_gpu as they are.
//
// The one-sort count (count_solid_gpu_t) needs 56-104 bytes a text position; the text itself is one byte a position.
// Here the text stays on the device and the canonical k-mers are counted range by range of the key space:
//   1. k_hist_keys    a histogram of the keys over their top bits (64-bit global bins, counted in LDS first);
//   2. plan_passes    (pass_plan.hpp) consecutive bins of at most C keys become a pass; a bin beyond C is histogrammed
//                     again on its next bits, down to the key's last bit — a single k-mer beyond C cannot be split;
//   3. per pass       k_extract_range writes the keys of the range, compacted (votes and prefix counts in a wave, one
//                     add on the cursor a wave and tile); sort, run heads, solid filter as in the
//                     one-sort count; the pass's solid k-mers are appended to the host array.
// Consecutive ranges one behind the other give the sorted set the single sort gives.
//
// Both kernels walk the text the same way (d_roll_tile): a workgroup stages 16 384 positions plus a halo in LDS with
// 16-byte loads, a thread owns 64 consecutive start positions and rolls the forward and the reverse-complement word by
// one base a position — k - 1 warm-up bases and 64 windows a thread instead of k byte loads and a d_revcomp a window.
// Run length and workgroup size: 256 threads x 64 positions is a 20 KiB tile (+ 16 KiB of bins in the histogram form), so
// four workgroups (16 waves) share a CU's 160 KiB with room to spare, and the warm-up is (k - 1) / 64 of the work.  A
// thread reads its run as 16-byte LDS words; runs are 64 bytes apart, which alone would put a 16-lane group of a
// ds_read_b128 on four slots — every run is therefore followed by one slot of padding (stride 80 bytes: 5 t mod 16 is a
// permutation of the slots).
#pragma once

#include <algorithm>
#include <cstdlib>

#include "pass_plan.hpp"

namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_RUN = 64;                       // start positions a thread
constexpr int PB_TILE = PB_THREADS * PB_RUN;     // start positions a workgroup and tile
constexpr int PB_HALO = 128;                     // >= kMaxK - 1, rounded to the run's 16-byte words
constexpr int PB_SLOTS = (PB_TILE + PB_HALO) / 16;
constexpr int PB_LDS_SLOTS = PB_SLOTS + PB_SLOTS / 4 + 1;  // one slot of padding behind every four
constexpr int PB_HIST_BITS = 12;
constexpr uint32_t PB_MAX_BINS = 1u << PB_HIST_BITS;
static_assert(PB_RUN % 16 == 0 && (g2s::kMaxK - 1 + 15) / 16 * 16 <= PB_HALO, "a thread reads whole 16-byte words inside the halo");

// a key range [lo, last], both ends included (no value follows the largest key of a full-width k-mer), as words
struct KeyRange {
  uint64_t lo[4], last[4];
};

template <class KT> __device__ __forceinline__ KT d_from_words(const uint64_t* w);
template <> __device__ __forceinline__ uint64_t d_from_words<uint64_t>(const uint64_t* w) { return w[0]; }
template <> __device__ __forceinline__ u128 d_from_words<u128>(const uint64_t* w) { return ((u128)w[1] << 64) | (u128)w[0]; }
template <> __device__ __forceinline__ u256 d_from_words<u256>(const uint64_t* w) {
  return u256(((u128)w[3] << 64) | (u128)w[2], ((u128)w[1] << 64) | (u128)w[0]);
}
// the low 2k bits set
template <class KT> __device__ __forceinline__ KT d_low_mask(int k);
template <> __device__ __forceinline__ uint64_t d_low_mask<uint64_t>(int k) { return k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1); }
template <> __device__ __forceinline__ u128 d_low_mask<u128>(int k) { return k >= 64 ? ~(u128)0 : (((u128)1 << (2 * k)) - 1); }
template <> __device__ __forceinline__ u256 d_low_mask<u256>(int k) { return (~u256()) >> (256 - 2 * k); }
// a base's code at bit `sh` (even)
template <class KT> __device__ __forceinline__ KT d_code_at(uint32_t c, int sh);
template <> __device__ __forceinline__ uint64_t d_code_at<uint64_t>(uint32_t c, int sh) { return (uint64_t)c << sh; }
template <> __device__ __forceinline__ u128 d_code_at<u128>(uint32_t c, int sh) { return (u128)c << sh; }
template <> __device__ __forceinline__ u256 d_code_at<u256>(uint32_t c, int sh) {
  return sh >= 128 ? u256((u128)c << (sh - 128), (u128)0) : u256((u128)0, (u128)c << sh);
}

// One tile of the text into LDS: 16-byte loads, a slot of padding behind every four.  `text` is readable to the end of
// the last tile's halo and holds an invalid character from the text's end on, so a window that runs off the end is
// invalid like one with an N.  The caller synchronises before the tile is read and before it is overwritten.
__device__ __forceinline__ void d_load_tile(const uint8_t* __restrict__ text, uint64_t tile, uint4* lds) {
  const uint4* src = (const uint4*)(text + tile * (uint64_t)PB_TILE);
  for (int q = threadIdx.x; q < PB_SLOTS; q += PB_THREADS) lds[q + (q >> 2)] = src[q];
}
// emit(valid, canonical k-mer) for each of the thread's PB_RUN start positions in the tile, every lane of the workgroup
// at the same step (emit may vote across the wave).  The count of valid characters in a row follows k_extract's rule:
// bit 3 of the byte set means invalid.
template <class KT, class Emit>
__device__ __forceinline__ void d_roll_tile(const uint4* lds, int k, Emit&& emit) {
  const KT mask = d_low_mask<KT>(k);
  const int top = 2 * (k - 1);
  const int steps = PB_RUN + k - 1;  // characters the thread reads: its windows' first to its last window's last
  KT f = 0, r = 0;
  int run = 0;
  const int q0 = (int)threadIdx.x * (PB_RUN / 16);
  for (int c = 0; c * 16 < steps; c++) {
    const int q = q0 + c;
    const uint4 v = lds[q + (q >> 2)];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t ch = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const uint32_t code = (ch >> 1) & 3u;
      run = (ch >> 3) & 1u ? 0 : run + 1;
      f = ((f << 2) | (KT)(uint64_t)code) & mask;
      r = (r >> 2) | d_code_at<KT>(code ^ 2u, top);
      const int i = c * 16 + j;  // the window [i - (k - 1), i] of the thread's characters ends here
      if (i >= k - 1 && i < steps) emit(run >= k, f < r ? f : r);
    }
  }
}

template <class KT>
__device__ __forceinline__ bool d_in_range(const KT& key, const KT& lo, const KT& last) { return !(key < lo) && !(last < key); }

// hist[b] += the valid windows whose canonical k-mer lies in [lo, last] and has (key >> shift) mod nbins == b.  The
// range is aligned to nbins << shift, so b counts from the range's start.  nbins <= PB_MAX_BINS, a power of two.
template <class KT>
__global__ __launch_bounds__(PB_THREADS) void k_hist_keys(const uint8_t* __restrict__ text, uint64_t ntiles, int k, KeyRange rg,
                                                          int shift, uint32_t nbins, unsigned long long* __restrict__ hist) {
  __shared__ uint4 tile[PB_LDS_SLOTS];
  __shared__ uint32_t bins[PB_MAX_BINS];  // (a workgroup counts fewer than 2^32 windows: ntiles / gridDim.x tiles of 2^14)
  for (uint32_t b = threadIdx.x; b < nbins; b += PB_THREADS) bins[b] = 0;
  const KT lo = d_from_words<KT>(rg.lo), last = d_from_words<KT>(rg.last);
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();  // (the tile's readers of the round before; the first round: the bins are zero)
    d_load_tile(text, t, tile);
    __syncthreads();
    d_roll_tile<KT>(tile, k, [&](bool ok, const KT& key) {
      if (ok && d_in_range(key, lo, last)) atomicAdd(&bins[(uint32_t)(key >> shift) & (nbins - 1u)], 1u);
    });
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += PB_THREADS)
    if (bins[b]) atomicAdd(&hist[b], (unsigned long long)bins[b]);
}

// keys[0 .. *cursor) = the canonical k-mers in [lo, last] of all valid windows, in no particular order.  A wave rolls
// its part of the tile twice: once to count its keys by votes, then — behind one add on the cursor for the wave and tile —
// to write them, each step's keys at the vote's prefix count.  (One add a step and wave, a single roll, was 8 times
// k_extract's time: 1.9 M adds on one address at 120 M positions.)  `cap` keys fit; the host compares *cursor with the
// histogram's count, and nothing is written beyond cap whatever the two say.
template <class KT>
__global__ __launch_bounds__(PB_THREADS) void k_extract_range(const uint8_t* __restrict__ text, uint64_t ntiles, int k, KeyRange rg,
                                                              KT* __restrict__ keys, uint64_t cap,
                                                              unsigned long long* __restrict__ cursor) {
  __shared__ uint4 tile[PB_LDS_SLOTS];
  const KT lo = d_from_words<KT>(rg.lo), last = d_from_words<KT>(rg.last);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();  // (the tile's readers of the round before)
    d_load_tile(text, t, tile);
    __syncthreads();
    uint32_t mine = 0;  // the wave's keys in this tile: the same in every lane
    d_roll_tile<KT>(tile, k, [&](bool ok, const KT& key) { mine += (uint32_t)__popcll(__ballot(ok && d_in_range(key, lo, last))); });
    if (mine == 0) continue;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(cursor, (unsigned long long)mine);
    at = __shfl(at, 0);
    d_roll_tile<KT>(tile, k, [&](bool ok, const KT& key) {
      const bool sel = ok && d_in_range(key, lo, last);
      const uint64_t votes = __ballot(sel);
      const uint64_t to = at + (uint64_t)__popcll(votes & below);
      if (sel && to < cap) keys[to] = key;
      at += (uint64_t)__popcll(votes);
    });
  }
}

}  // namespace

namespace g2s {

template <class KT> static void key_words(const KT& x, uint64_t* w);
template <> void key_words<uint64_t>(const uint64_t& x, uint64_t* w) { w[0] = x; w[1] = w[2] = w[3] = 0; }
template <> void key_words<u128>(const u128& x, uint64_t* w) { w[0] = (uint64_t)x; w[1] = (uint64_t)(x >> 64); w[2] = w[3] = 0; }
template <> void key_words<u256>(const u256& x, uint64_t* w) { for (int i = 0; i < 4; i++) w[i] = x.word(i); }

// The text on the device: every sequence followed by one 'N', through two page-locked staging buffers of `piece` bytes
// that are filled from the caller's sequences while the other one's copy is under way.
static bool upload_text_staged(uint8_t* d_text, const std::vector<std::pair<const char*, uint64_t>>& seqs, uint64_t T, size_t piece,
                               std::string* why) {
  PinMem buf[2];
  DevEvent done[2];
  bool used[2] = {false, false};
  for (int b = 0; b < 2; b++) {
    G2S_HIP_TRY(buf[b].alloc(piece));
    G2S_HIP_TRY(done[b].create());
  }
  size_t si = 0;
  uint64_t off = 0, sent = 0;  // off == the sequence's length: its separator comes next
  for (int b = 0; sent < T; b ^= 1) {
    if (used[b]) G2S_HIP_TRY(hipEventSynchronize(done[b].e));
    uint8_t* dst = (uint8_t*)buf[b].p;
    size_t fill = 0;
    while (fill < piece && si < seqs.size()) {
      const uint64_t len = seqs[si].second;
      if (off < len) {
        const size_t n = (size_t)std::min<uint64_t>(len - off, piece - fill);
        memcpy(dst + fill, seqs[si].first + off, n);
        fill += n;
        off += n;
      } else {
        dst[fill++] = 'N';
        si++;
        off = 0;
      }
    }
    G2S_HIP_TRY(hipMemcpyAsync(d_text + sent, dst, fill, hipMemcpyHostToDevice, 0));
    G2S_HIP_TRY(hipEventRecord(done[b].e, 0));
    used[b] = true;
    sent += fill;
  }
  G2S_HIP_TRY(hipStreamSynchronize(0));
  return true;
}

template <class KT>
struct SolidPasses {
  const uint8_t* d_text = nullptr;
  uint64_t ntiles = 0, cap = 0;
  int k = 0, solid = 1;
  std::vector<KT>* out = nullptr;
  std::string* why = nullptr;
  DevMem d_hist, d_cursor;
  uint32_t passes = 0, refined = 0;
  uint64_t max_pass_keys = 0, valid_keys = 0;

  static KeyRange range_of(const KT& lo, const KT& last) {
    KeyRange rg;
    key_words<KT>(lo, rg.lo);
    key_words<KT>(last, rg.last);
    return rg;
  }
  // With reach records the passes' solid keys stay on the device, one behind the other in d_table (graph_reach.h searches
  // that table; it may hold any number of keys the device has room for).
  bool keep_on_device = false;
  DevMem d_table;
  uint64_t table_n = 0, table_cap = 0;
  // (graph_build refuses a host-bound set of 2^30 k-mers: no need to finish it; a device-held table is not the graph's set)
  bool full() const { return !keep_on_device && out->size() >= ((size_t)1 << 30); }
  bool append_on_device(const KT* d_keys, uint64_t n_new, uint64_t count) {
    if (table_n + n_new > table_cap) {
      // (room for the passes to come at this pass's share of solid keys; doubling behind that)
      uint64_t want = std::max<uint64_t>(table_n + n_new, 2 * table_cap);
      if (table_cap == 0 && count < valid_keys) want = std::max<uint64_t>(want, (uint64_t)(1.05 * (double)n_new / (double)count * (double)valid_keys) + 1024);
      DevMem bigger;
      G2S_HIP_TRY(bigger.alloc((size_t)want * sizeof(KT)));
      if (table_n) G2S_HIP_TRY(hipMemcpy(bigger.p, d_table.p, (size_t)table_n * sizeof(KT), hipMemcpyDeviceToDevice));
      d_table.free();
      d_table = std::move(bigger);
      table_cap = want;
    }
    G2S_HIP_TRY(hipMemcpy(d_table.as<KT>() + table_n, d_keys, (size_t)n_new * sizeof(KT), hipMemcpyDeviceToDevice));
    table_n += n_new;
    return true;
  }

  // the keys below `prefix`'s bits that level `level` and the levels above it have fixed: histogram, plan, passes
  bool run_level(int level, const KT& prefix) {
    const int bits_left = 2 * k - level * PB_HIST_BITS;
    const int hb = std::min(PB_HIST_BITS, bits_left), shift = bits_left - hb;
    const uint32_t nbins = 1u << hb;
    // bins [b0, b1) of this level hold the keys [first_key(b0), last_key(b1)]; prefix's low hb + shift bits are zero
    auto first_key = [&](uint32_t b) { return prefix | (KT((uint64_t)b) << shift); };
    auto last_key = [&](uint32_t b1) { return prefix | ((KT((uint64_t)b1) << shift) - KT((uint64_t)1)); };
    G2S_HIP_TRY(hipMemset(d_hist.p, 0, (size_t)nbins * 8));
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 1024);
    hipLaunchKernelGGL(k_hist_keys<KT>, dim3(grid), dim3(PB_THREADS), 0, 0, d_text, ntiles, k,
                       range_of(prefix, last_key(nbins)), shift, nbins, d_hist.as<unsigned long long>());
    G2S_HIP_TRY(hipGetLastError());
    std::vector<uint64_t> hist((size_t)nbins);
    G2S_HIP_TRY(hipMemcpy(hist.data(), d_hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost));
    if (level == 0)
      for (uint64_t h : hist) valid_keys += h;
    std::vector<uint32_t> first_bin;
    const uint32_t np = plan_passes(hist.data(), nbins, cap, &first_bin, nullptr);
    for (uint32_t p = 0; p < np && !full(); p++) {
      const uint32_t b0 = first_bin[p], b1 = first_bin[p + 1];
      uint64_t count = 0;
      for (uint32_t b = b0; b < b1; b++) count += hist[b];
      if (count == 0) continue;
      if (count > cap) {  // (one bin: plan_passes)
        if (shift == 0) {
          if (why) *why = "one k-mer occurs " + std::to_string(count) + " times, more than the " + std::to_string(cap) + " keys of a pass";
          return false;
        }
        refined++;
        if (!run_level(level + 1, first_key(b0))) return false;
      } else if (!run_pass(first_key(b0), last_key(b1), count)) {
        return false;
      }
    }
    return true;
  }

  // extract, sort, run lengths, solid filter on the `count` keys in [lo, last]
  bool run_pass(const KT& lo, const KT& last, uint64_t count) {
    const dim3 blk(256), grdN((unsigned)((count + 255) / 256));
    DevMem d_keys, d_alt, d_flag, d_pos, d_hidx, d_keep, d_kpos, d_out, d_misc;
    G2S_HIP_TRY(d_keys.alloc((size_t)count * sizeof(KT)));
    G2S_HIP_TRY(d_misc.alloc(16));
    G2S_HIP_TRY(hipMemset(d_cursor.p, 0, 8));
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 2048);
    hipLaunchKernelGGL(k_extract_range<KT>, dim3(grid), dim3(PB_THREADS), 0, 0, d_text, ntiles, k, range_of(lo, last),
                       d_keys.as<KT>(), count, d_cursor.as<unsigned long long>());
    G2S_HIP_TRY(hipGetLastError());
    uint64_t got = 0;
    G2S_HIP_TRY(hipMemcpy(&got, d_cursor.p, 8, hipMemcpyDeviceToHost));
    if (got != count) {
      if (why) *why = "a pass extracted " + std::to_string(got) + " keys where the histogram counted " + std::to_string(count);
      return false;
    }
    const KT* sorted = nullptr;
    if constexpr (sizeof(KT) == 8) {
      Scratch d_tmp;
      G2S_HIP_TRY(d_alt.alloc((size_t)count * 8));
      G2S_HIP_TRY(radix_sort_keys(d_tmp, d_keys.as<uint64_t>(), d_alt.as<uint64_t>(), (size_t)count, (unsigned)(2 * k)));
      d_keys.free();
      sorted = d_alt.as<KT>();
    } else {
      if (!sort_keyed_gpu<KT>(d_keys, nullptr, count, d_alt, nullptr, why)) return false;
      sorted = d_alt.as<KT>();
    }
    // ---- runs of equal keys -> the k-mers seen at least `solid` times (count_solid_gpu_t, on this pass's keys)
    G2S_HIP_TRY(d_flag.alloc((size_t)count * 4));
    G2S_HIP_TRY(d_pos.alloc((size_t)count * 4));
    hipLaunchKernelGGL(k_heads<KT>, grdN, blk, 0, 0, sorted, count, d_flag.as<uint32_t>());
    Scratch d_tmp2, d_tmp3;
    uint32_t nheads = 0, n_solid = 0;
    G2S_HIP_TRY(scan_total(d_tmp2, (const uint32_t*)d_flag.p, d_pos.as<uint32_t>(), (size_t)count, &nheads));
    if (nheads) {
      G2S_HIP_TRY(d_hidx.alloc((size_t)nheads * 4));
      G2S_HIP_TRY(d_keep.alloc((size_t)nheads * 4));
      G2S_HIP_TRY(d_kpos.alloc((size_t)nheads * 4));
      G2S_HIP_TRY(hipMemset(d_misc.p, 0, 16));
      hipLaunchKernelGGL(k_head_index<KT>, grdN, blk, 0, 0, sorted, (const uint32_t*)d_flag.p, (const uint32_t*)d_pos.p, count,
                         d_hidx.as<uint32_t>(), d_misc.as<uint32_t>());
      uint32_t n_valid = 0;
      G2S_HIP_TRY(hipMemcpy(&n_valid, d_misc.p, 4, hipMemcpyDeviceToHost));
      const dim3 grdH((nheads + 255) / 256);
      hipLaunchKernelGGL(k_solid_flag, grdH, blk, 0, 0, (const uint32_t*)d_hidx.p, nheads, n_valid, (uint32_t)std::max(1, solid),
                         d_keep.as<uint32_t>());
      G2S_HIP_TRY(scan_total(d_tmp3, (const uint32_t*)d_keep.p, d_kpos.as<uint32_t>(), (size_t)nheads, &n_solid));
      if (n_solid) {
        G2S_HIP_TRY(d_out.alloc((size_t)n_solid * sizeof(KT)));
        hipLaunchKernelGGL(k_compact<KT>, grdH, blk, 0, 0, sorted, (const uint32_t*)d_hidx.p, (const uint32_t*)d_keep.p,
                           (const uint32_t*)d_kpos.p, nheads, d_out.as<KT>());
      }
    }
    G2S_HIP_TRY(hipGetLastError());
    if (n_solid && keep_on_device) {
      if (!append_on_device(d_out.as<KT>(), n_solid, count)) return false;
    } else if (n_solid) {
      const size_t at = out->size();
      // (room for the passes to come at this pass's share of solid keys, so that the array is not copied as it grows)
      if (passes == 0 && count < valid_keys)
        out->reserve((size_t)std::min<double>((double)(1ull << 30), 1.05 * (double)n_solid / (double)count * (double)valid_keys));
      out->resize(at + n_solid);
      G2S_HIP_TRY(hipMemcpy(out->data() + at, d_out.p, (size_t)n_solid * sizeof(KT), hipMemcpyDeviceToHost));
    }
    passes++;
    max_pass_keys = std::max(max_pass_keys, count);
    return true;
  }
};

static uint64_t env_u64(const char* name) {
  const char* s = getenv(name);
  return s && *s ? strtoull(s, nullptr, 10) : 0;
}
// G2S_BUILD_PASS_KEYS=N: the pass form whatever the size, N keys a pass
static bool solid_passes_forced() { return env_u64("G2S_BUILD_PASS_KEYS") != 0; }

// The pass form of count_solid_gpu_t (the device is set; T > 0 positions; per_key = its bytes a sorted key).  false with a
// reason (g untouched) when the text does not fit beside a pass or one k-mer alone is more than a pass.  g.bucket stays
// empty: finish_graph builds the prefix index as for a host-made set.
template <class KT>
static bool count_solid_passes_gpu_t(Graph& g, std::vector<KT>& out, const BuildInput& in, int solid, uint64_t T, double per_key,
                                     std::string* why, SolidCountInfo* info) {
  const uint64_t ntiles = (T + PB_TILE - 1) / PB_TILE;
  // (a text that is on the device already has this padding and takes no further room: reads_text.h)
  const uint64_t text_bytes = in.text ? 0 : ntiles * (uint64_t)PB_TILE + PB_HALO;
  if (in.text && (device_text_bytes(T) != ntiles * (uint64_t)PB_TILE + PB_HALO || in.text->capacity < device_text_bytes(T))) {
    if (why) *why = "the resident text lacks the passes' padding";
    return false;
  }
  size_t free_b = 0, total_b = 0;
  G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const uint64_t cap_max = 1ull << 31;  // (a pass's keys are indexed in 32 bits)
  uint64_t cap = std::min(env_u64("G2S_BUILD_PASS_KEYS"), cap_max);
  const bool forced = cap != 0;
  // (unforced, a pass of fewer than 2^24 keys is not worth its walk over the text)
  const double need = (double)text_bytes + (forced ? (double)cap : (double)(1u << 24)) * per_key;
  if (need > 0.5 * (double)free_b) { if (why) *why = "text does not fit on the device beside a pass"; return false; }
  DevMem d_text;
  if (!in.text) {
    G2S_HIP_TRY(d_text.alloc((size_t)text_bytes));
    G2S_HIP_TRY(hipMemset(d_text.as<uint8_t>() + T, 'N', (size_t)(text_bytes - T)));
    const uint64_t piece = env_u64("G2S_BUILD_PIECE_BYTES");
    if (!upload_text_staged(d_text.as<uint8_t>(), *in.seqs, T, (size_t)(piece ? std::max<uint64_t>(piece, 16) : std::min<uint64_t>(32u << 20, T)), why)) return false;
  }
  if (!forced) {
    G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // (with reach records the solid keys stay on the device: a quarter of the free memory is left to that table, whose
    // growth holds the old and the new array at once)
    cap = (uint64_t)((in.reach ? 0.25 : 0.5) * (double)free_b / per_key);
  }
  cap = std::min(cap, cap_max);
  std::vector<KT> kept;
  SolidPasses<KT> sp;
  sp.d_text = in.text ? in.text->d_text : d_text.as<uint8_t>();
  sp.ntiles = ntiles;
  sp.cap = cap;
  sp.k = g.k;
  sp.solid = solid;
  sp.out = &kept;
  sp.why = why;
  sp.keep_on_device = in.reach != nullptr;
  G2S_HIP_TRY(sp.d_hist.alloc((size_t)PB_MAX_BINS * 8));
  G2S_HIP_TRY(sp.d_cursor.alloc(8));
  if (!sp.run_level(0, KT((uint64_t)0))) return false;
  if (in.text) free_device_text(in.text);  // (the passes were its last readers; d_text goes at the function's end)
  if (in.reach) {  // the kept part of the device-held table is the set (graph_reach.h)
    d_text.free();
    GraphReachInfo rinfo;
    uint64_t nkept = 0;
    DevMem d_kept;
    if (sp.table_n && !reach_on_device<KT>(sp.d_table.template as<KT>(), sp.table_n, g.k, *in.reach, d_kept, &nkept, why, &rinfo)) return false;
    if (!sp.table_n) { rinfo.records = in.reach->records; rinfo.seeds = in.reach->seed.size(); rinfo.on_device = 1; }
    rinfo.passes = sp.passes;
    set_graph_reach_info(rinfo);
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s]   reach: %llu of %llu k-mers kept on the GPU, %u levels, the queue grown %u times\n",
              (unsigned long long)nkept, (unsigned long long)sp.table_n, rinfo.levels, rinfo.regrowths);
    if (nkept < graph_max_kmers() && nkept) {
      kept.resize((size_t)nkept);
      G2S_HIP_TRY(hipMemcpy(kept.data(), d_kept.p, (size_t)nkept * sizeof(KT), hipMemcpyDeviceToHost));
    }
    out.swap(kept);
    g.n = nkept;  // (at or over the cap: graph_build refuses it, nothing came down)
    g.bucket.clear();
    if (info) {
      info->passes = sp.passes;
      info->refined_bins = sp.refined;
      info->max_pass_keys = sp.max_pass_keys;
    }
    return true;
  }
  if (getenv("G2S_DEBUG"))
    fprintf(stderr, "[g2s]   k-mer set in %u key-range passes of at most %llu keys (largest %llu, %u bins refined, %llu of %llu positions valid)\n",
            sp.passes, (unsigned long long)cap, (unsigned long long)sp.max_pass_keys, sp.refined,
            (unsigned long long)sp.valid_keys, (unsigned long long)T);
  out.swap(kept);
  g.n = out.size();
  g.bucket.clear();
  if (info) {
    info->passes = sp.passes;
    info->refined_bins = sp.refined;
    info->max_pass_keys = sp.max_pass_keys;
  }
  return true;
}

}  // namespace g2s
