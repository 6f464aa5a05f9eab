// gap2seq_amd/csrc/readfilter_gpu.hip — the joins of the batched read filter (readfilter_gaps.cpp) on the GPU.
//
// In: one row per BAM record (reference, position, end position, flag, std::hash of the read's name and of its
// mate's), copied up from the host walk's FilterRows or left in device memory by pass A's kernels (bam_rows.hip), and
// three windows a gap (readfilter_gaps.hpp).  Out: lists 1 and 2 as
// (gap << 32 | row) pairs in ascending order.  Steps, each sized before it is written (count, exclusive scan, write):
//   1. k_bits         bit = hash % (5 * records) of every name and mate name, in place (64-bit modulo)
//   2. index          (ref_id, pos) keys radix-sorted with their rows (rocPRIM, as the set build in dbg_gpu.hip); a
//                     window's rows are the keys in [(tid, beg - longest span + 1), (tid, end)) — two binary searches
//                     — whose end position is > beg.  No order of the file is assumed.
//   3. k_gap<0>       per gap (one wave a gap), the (bit << 29 | gap) keys of the mate-unmapped rows in its left and
//                     right windows; sorted and de-duplicated: U
//   4. k_mates        per row, the keys of U whose bit is the row's mate's bit: one list 1 pair each
//   5. k_gap<1>       per gap, the rows in its flank window whose own (bit, gap) key is not in U: list 2
//   6. both lists radix-sorted: (gap, row) order, and row order is file order.
// Every pair count is checked against the cap (FilterJoin::max_pairs) before its buffer exists.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g2s.h"
#include "hip_host.h"
#include "readfilter_gaps.hpp"

namespace {

constexpr int kWave = 64;

int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? G2S_ERR_NOMEM : G2S_ERR_HIP; }  // (G2S_HIP_TRY_CODE)

__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t* __restrict__ a, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// (readfilter_gaps.hpp: filter_index_key)
__device__ __forceinline__ uint64_t index_key(int32_t tid, int64_t p) {
  p = p < (int64_t)INT32_MIN ? (int64_t)INT32_MIN : p > (int64_t)INT32_MAX + 1 ? (int64_t)INT32_MAX + 1 : p;
  return ((uint64_t)(uint32_t)tid << 32) + (uint64_t)(p - (int64_t)INT32_MIN);
}

__global__ void k_bits(uint64_t* __restrict__ h_own, uint64_t* __restrict__ h_mate, uint32_t nr, uint64_t bits,
                       const int32_t* __restrict__ ref_id, const int32_t* __restrict__ pos, uint64_t* __restrict__ ikey,
                       uint32_t* __restrict__ irow) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nr) return;
  h_own[r] %= bits;
  h_mate[r] %= bits;
  ikey[r] = index_key(ref_id[r], pos[r]);
  irow[r] = r;
}

// MODE 0: the (bit << 29 | gap) keys of the mate-unmapped rows of windows 0 and 1 (left, right);
// MODE 1: the (gap << 32 | row) pairs of the rows of window 2 (around) whose (bit, gap) key is not in U.
// WRITE false: cnt[g] = the number of items; WRITE true: the items at out[off[g] ...].  One wave a gap: every lane
// walks the same ranges, so the ballots are uniform and both launches visit the items in the same order.
template <int MODE, bool WRITE>
__global__ void __launch_bounds__(kWave) k_gap(const g2s::FilterWindow* __restrict__ win, uint32_t n,
                                               const uint64_t* __restrict__ ikey, const uint32_t* __restrict__ irow, uint64_t nr,
                                               const int64_t* __restrict__ endp, const uint32_t* __restrict__ flag,
                                               const uint64_t* __restrict__ b_own, const uint64_t* __restrict__ U, uint64_t nu,
                                               int64_t max_span, uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                               uint64_t* __restrict__ out) {
  const uint32_t g = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (g >= n) return;
  uint64_t at = WRITE ? off[g] : 0;
  for (int w = MODE == 0 ? 0 : 2; w < (MODE == 0 ? 2 : 3); w++) {
    const g2s::FilterWindow q = win[3 * (size_t)g + w];
    if (q.tid < 0 || q.beg >= q.end) continue;
    const uint64_t lo = lower_bound_u64(ikey, nr, index_key(q.tid, q.beg - max_span + 1));
    const uint64_t hi = lower_bound_u64(ikey, nr, index_key(q.tid, q.end));
    for (uint64_t i0 = lo; i0 < hi; i0 += kWave) {
      const uint64_t i = i0 + lane;
      bool take = false;
      uint64_t v = 0;
      if (i < hi) {
        const uint32_t r = irow[i];
        if (endp[r] > q.beg) {
          const uint64_t key = b_own[r] << g2s::kFilterGapBits | g;
          if (MODE == 0) {
            take = (flag[r] & g2s::BAM_MATE_UNMAPPED) != 0;
            v = key;
          } else {
            const uint64_t j = lower_bound_u64(U, nu, key);
            take = !(j < nu && U[j] == key);
            v = (uint64_t)g << 32 | r;
          }
        }
      }
      const uint64_t mask = __ballot(take);
      if (WRITE && take) out[at + __popcll(mask & (((uint64_t)1 << lane) - 1))] = v;
      at += __popcll(mask);
    }
  }
  if (!WRITE && lane == 0) cnt[g] = at;
}

// list 1: the keys of U with the row's mate's bit (U is sorted by bit, then gap)
template <bool WRITE>
__global__ void k_mates(const uint64_t* __restrict__ b_mate, uint32_t nr, const uint64_t* __restrict__ U, uint64_t nu,
                        uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint64_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nr) return;
  const uint64_t m = b_mate[r];
  const uint64_t lo = lower_bound_u64(U, nu, m << g2s::kFilterGapBits);
  const uint64_t hi = lower_bound_u64(U, nu, (m + 1) << g2s::kFilterGapBits);
  if (!WRITE) { cnt[r] = hi - lo; return; }
  const uint64_t o = off[r];
  for (uint64_t i = lo; i < hi; i++) out[o + (i - lo)] = (U[i] & g2s::kFilterGapMask) << 32 | r;
}

}  // namespace

namespace g2s {

bool filter_device_usable(int device) {
  int ndev = 0;
  if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return false;
  hipDeviceProp_t prop;
  return hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

int filter_join_device(FilterJoin& j, int device, std::string* err) {
  auto over_cap = [&](uint64_t count) {
    if (count > j.max_pairs) *err = "more filter pairs than the cap (G2S_FILTER_MAX_PAIRS)";
    return count > j.max_pairs;
  };
  const FilterRows& R = *j.rows;
  const DeviceRows* DR = j.device_rows;
  const uint64_t nr = DR ? DR->n : R.size();
  const int64_t max_span = DR ? DR->max_span : R.max_span;
  const uint32_t n = (uint32_t)j.gaps();
  j.list1.clear();
  j.list2.clear();
  G2S_HIP_TRY_CODE(hipSetDevice(device));
  if (!nr || !j.bits || !n) return G2S_OK;  // (no records: the filter is empty and no window holds anything)
  const dim3 blk(256), grdR((unsigned)((nr + 255) / 256));
  // ---- rows up
  DevMem d_ref, d_pos, d_end, d_flag, d_own, d_mate, d_ikey, d_irow, d_ikey2, d_irow2, d_win;
  Scratch d_tmp;
  G2S_HIP_TRY_CODE(d_win.alloc(j.win.size() * sizeof(FilterWindow)));
  G2S_HIP_TRY_CODE(hipMemcpy(d_win.p, j.win.data(), j.win.size() * sizeof(FilterWindow), hipMemcpyHostToDevice));
  if (!DR) {
    G2S_HIP_TRY_CODE(d_ref.alloc(nr * 4));
    G2S_HIP_TRY_CODE(d_pos.alloc(nr * 4));
    G2S_HIP_TRY_CODE(d_end.alloc(nr * 8));
    G2S_HIP_TRY_CODE(d_flag.alloc(nr * 4));
    G2S_HIP_TRY_CODE(d_own.alloc(nr * 8));
    G2S_HIP_TRY_CODE(d_mate.alloc(nr * 8));
    G2S_HIP_TRY_CODE(hipMemcpy(d_ref.p, R.ref_id.data(), nr * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY_CODE(hipMemcpy(d_pos.p, R.pos.data(), nr * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY_CODE(hipMemcpy(d_end.p, R.end.data(), nr * 8, hipMemcpyHostToDevice));
    G2S_HIP_TRY_CODE(hipMemcpy(d_flag.p, R.flag.data(), nr * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY_CODE(hipMemcpy(d_own.p, R.h_own.data(), nr * 8, hipMemcpyHostToDevice));
    G2S_HIP_TRY_CODE(hipMemcpy(d_mate.p, R.h_mate.data(), nr * 8, hipMemcpyHostToDevice));
  }
  // (rows that pass A left on the device are read where they lie, and stay their owner's)
  const int32_t* p_ref = DR ? DR->ref_id : d_ref.as<int32_t>();
  const int32_t* p_pos = DR ? DR->pos : d_pos.as<int32_t>();
  const int64_t* p_end = DR ? DR->end : d_end.as<int64_t>();
  const uint32_t* p_flag = DR ? DR->flag : d_flag.as<uint32_t>();
  uint64_t* p_own = DR ? DR->h_own : d_own.as<uint64_t>();
  uint64_t* p_mate = DR ? DR->h_mate : d_mate.as<uint64_t>();
  // ---- 1, 2: bits, and the index sorted
  G2S_HIP_TRY_CODE(d_ikey.alloc(nr * 8));
  G2S_HIP_TRY_CODE(d_irow.alloc(nr * 4));
  G2S_HIP_TRY_CODE(d_ikey2.alloc(nr * 8));
  G2S_HIP_TRY_CODE(d_irow2.alloc(nr * 4));
  hipLaunchKernelGGL(k_bits, grdR, blk, 0, 0, p_own, p_mate, (uint32_t)nr, j.bits, p_ref, p_pos, d_ikey.as<uint64_t>(),
                     d_irow.as<uint32_t>());
  G2S_HIP_TRY_CODE(hipGetLastError());
  G2S_HIP_TRY_CODE(radix_sort_pairs(d_tmp, d_ikey.as<uint64_t>(), d_ikey2.as<uint64_t>(), d_irow.as<uint32_t>(),
                                    d_irow2.as<uint32_t>(), (size_t)nr));
  const uint64_t* ikey = d_ikey2.as<uint64_t>();
  const uint32_t* irow = d_irow2.as<uint32_t>();
  DevMem d_misc;
  G2S_HIP_TRY_CODE(d_misc.alloc(16));
  G2S_HIP_TRY_CODE(hipMemset(d_misc.p, 0, 16));
  // ---- 3: every gap's filter keys: count, scan, write, sort, unique
  DevMem d_gcnt, d_goff, d_bk, d_bk2, d_U;
  G2S_HIP_TRY_CODE(d_gcnt.alloc((size_t)n * 8));
  G2S_HIP_TRY_CODE(d_goff.alloc((size_t)n * 8));
  hipLaunchKernelGGL((k_gap<0, false>), dim3(n), dim3(kWave), 0, 0, d_win.as<FilterWindow>(), n, ikey, irow, nr,
                     p_end, p_flag, p_own, (const uint64_t*)nullptr, (uint64_t)0,
                     max_span, d_gcnt.as<uint64_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr);
  G2S_HIP_TRY_CODE(hipGetLastError());
  uint64_t nb = 0;
  G2S_HIP_TRY_CODE(scan_total(d_gcnt.as<const uint64_t>(), d_goff.as<uint64_t>(), n, &nb));
  if (over_cap(nb)) return G2S_ERR_NOMEM;
  uint64_t nu = 0;
  G2S_HIP_TRY_CODE(d_U.alloc(nb * 8));
  if (nb) {
    G2S_HIP_TRY_CODE(d_bk.alloc(nb * 8));
    G2S_HIP_TRY_CODE(d_bk2.alloc(nb * 8));
    hipLaunchKernelGGL((k_gap<0, true>), dim3(n), dim3(kWave), 0, 0, d_win.as<FilterWindow>(), n, ikey, irow, nr,
                       p_end, p_flag, p_own, (const uint64_t*)nullptr,
                       (uint64_t)0, max_span, (uint64_t*)nullptr, d_goff.as<const uint64_t>(), d_bk.as<uint64_t>());
    G2S_HIP_TRY_CODE(hipGetLastError());
    Scratch s, s2;
    G2S_HIP_TRY_CODE(radix_sort_keys(s, d_bk.as<uint64_t>(), d_bk2.as<uint64_t>(), (size_t)nb));
    G2S_HIP_TRY_CODE(unique(s2, d_bk2.as<uint64_t>(), d_U.as<uint64_t>(), d_misc.as<uint64_t>(), (size_t)nb));
    G2S_HIP_TRY_CODE(hipMemcpy(&nu, d_misc.p, 8, hipMemcpyDeviceToHost));
  }
  const uint64_t* U = d_U.as<uint64_t>();
  // ---- 4: list 1: count per row, scan, write
  uint64_t n1 = 0;
  DevMem d_l1, d_l1s;
  if (nu) {
    DevMem d_rcnt, d_roff;
    G2S_HIP_TRY_CODE(d_rcnt.alloc(nr * 8));
    G2S_HIP_TRY_CODE(d_roff.alloc(nr * 8));
    hipLaunchKernelGGL((k_mates<false>), grdR, blk, 0, 0, p_mate, (uint32_t)nr, U, nu, d_rcnt.as<uint64_t>(),
                       (const uint64_t*)nullptr, (uint64_t*)nullptr);
    G2S_HIP_TRY_CODE(hipGetLastError());
    G2S_HIP_TRY_CODE(scan_total(d_rcnt.as<const uint64_t>(), d_roff.as<uint64_t>(), nr, &n1));
    if (over_cap(nb + n1)) return G2S_ERR_NOMEM;
    if (n1) {
      G2S_HIP_TRY_CODE(d_l1.alloc(n1 * 8));
      G2S_HIP_TRY_CODE(d_l1s.alloc(n1 * 8));
      hipLaunchKernelGGL((k_mates<true>), grdR, blk, 0, 0, p_mate, (uint32_t)nr, U, nu, (uint64_t*)nullptr,
                         d_roff.as<const uint64_t>(), d_l1.as<uint64_t>());
      G2S_HIP_TRY_CODE(hipGetLastError());
    }
  }
  // ---- 5: list 2: count per gap, scan, write
  uint64_t n2 = 0;
  DevMem d_l2, d_l2s;
  hipLaunchKernelGGL((k_gap<1, false>), dim3(n), dim3(kWave), 0, 0, d_win.as<FilterWindow>(), n, ikey, irow, nr,
                     p_end, p_flag, p_own, U, nu, max_span,
                     d_gcnt.as<uint64_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr);
  G2S_HIP_TRY_CODE(hipGetLastError());
  G2S_HIP_TRY_CODE(scan_total(d_gcnt.as<const uint64_t>(), d_goff.as<uint64_t>(), n, &n2));
  if (over_cap(nb + n1 + n2)) return G2S_ERR_NOMEM;
  if (n2) {
    G2S_HIP_TRY_CODE(d_l2.alloc(n2 * 8));
    G2S_HIP_TRY_CODE(d_l2s.alloc(n2 * 8));
    hipLaunchKernelGGL((k_gap<1, true>), dim3(n), dim3(kWave), 0, 0, d_win.as<FilterWindow>(), n, ikey, irow, nr,
                       p_end, p_flag, p_own, U, nu, max_span, (uint64_t*)nullptr,
                       d_goff.as<const uint64_t>(), d_l2.as<uint64_t>());
    G2S_HIP_TRY_CODE(hipGetLastError());
  }
  // ---- 6: both lists in (gap, row) order, down
  int end_bit = 33;
  while (end_bit < 64 && ((uint64_t)1 << (end_bit - 32)) < (uint64_t)n) end_bit++;
  for (int l = 0; l < 2; l++) {
    const uint64_t m = l == 0 ? n1 : n2;
    if (!m) continue;
    uint64_t* in = (l == 0 ? d_l1 : d_l2).as<uint64_t>();
    uint64_t* outp = (l == 0 ? d_l1s : d_l2s).as<uint64_t>();
    Scratch s;
    G2S_HIP_TRY_CODE(radix_sort_keys(s, in, outp, (size_t)m, end_bit));
    std::vector<uint64_t>& dst = l == 0 ? j.list1 : j.list2;
    dst.resize((size_t)m);
    G2S_HIP_TRY_CODE(hipMemcpy(dst.data(), outp, m * 8, hipMemcpyDeviceToHost));
  }
  G2S_HIP_TRY_CODE(hipDeviceSynchronize());
  return G2S_OK;
}

}  // namespace g2s
