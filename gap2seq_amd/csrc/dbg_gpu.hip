// gap2seq_amd/csrc/dbg_gpu.hip — the graph build after the solid k-mer set, on the GPU.
//
// The build (replaces gatb Graph::create, /root/reference/src/Gap2Seq.cpp:193-219) has four
// steps after the sorted set of solid canonical k-mers exists (dbg.cpp: count_solid):
//   1. successor table in sorted-rank space: 8 neighbour k-mers per k-mer, each a binary
//      search inside its prefix bucket (k_succ; 64-, 128- and 256-bit k-mers).  At even k a k-mer
//      can be its own reverse complement: such a palindrome exists on strand 1 only, and the
//      same searches also fill an explicit predecessor table (pred(v) = succ(v^1)^1 does not
//      hold next to a palindrome); odd k allocates and writes no such table;
//   2. numbering along maximal non-branching paths.  On the host this is one dependent,
//      cache-missing load per k-mer (0.35 s of a 0.49 s build at 3 Mbp, 11.7 s of 16.6 s at
//      60 Mbp); here it is list ranking by pointer jumping:
//        nxt[v]   the successor of oriented node v when the edge is unitig-internal (same
//                 predicate as the host's `step`), else INVALID;
//        chains   every unitig is two mirrored chains (v -> w  <=>  w^1 -> v^1); a chain's
//                 head is the node without an internal predecessor;
//        ranking  pd[v] = (predecessor, distance) is squared log2(longest unitig) times
//                 until it holds (head, distance from head);
//        ids      of the two mirrored chains the one with the smaller head is kept; kept
//                 heads take consecutive id ranges in head order (exclusive scan of the
//                 chain lengths), node id = base[head] + distance, orientation bit = the
//                 node's strand on that chain.
//      Circular unitigs have no head; the host walk numbers them after the rest.
//      A palindrome is always a unitig of its own (its strand-0 row is empty, so no edge at it
//      passes the predicate's test that the edge back leads to v^1); k_keep gives such a k-mer the
//      strand the host walk would start on.
//   3. the tables (at even k both) permuted into id space + the last base of every oriented node
//      (k_remap);
//   4. the unitig-start bitmap (k_ustart).
// The id-space table and the bitmap stay on the device: they are the graph's copy for the
// fill path.  All of it is HBM-bound random access: 0.05 s at 3 Mbp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "dbg.hpp"
#include "hip_host.h"
#include "reads_text.h"

namespace {

constexpr uint32_t INV = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t only_succ(const uint32_t* __restrict__ succ, uint32_t v, uint32_t* deg) {
  const uint4 r = *(const uint4*)(succ + (size_t)v * 4);
  const uint32_t d = (r.x != INV) + (r.y != INV) + (r.z != INV) + (r.w != INV);
  *deg = d;
  return r.x != INV ? r.x : r.y != INV ? r.y : r.z != INV ? r.z : r.w;
}

// the unique continuation v -> w when the edge is unitig-internal (dbg.cpp: step)
__global__ void k_next(const uint32_t* __restrict__ succ, uint32_t n2, uint32_t* __restrict__ nxt) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2) return;
  uint32_t deg, w = only_succ(succ, v, &deg), out = INV;
  if (deg == 1 && (w >> 1) != (v >> 1)) {
    uint32_t dback, back = only_succ(succ, w ^ 1u, &dback);  // in-degree of w
    if (dback == 1 && back == (v ^ 1u)) out = w;
  }
  nxt[v] = out;
}

__global__ void k_init(const uint32_t* __restrict__ nxt, uint32_t n2, uint64_t* __restrict__ pd) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2) return;
  const uint32_t m = nxt[v ^ 1u];  // v has an internal predecessor p  <=>  v^1 -> p^1 is internal
  pd[v] = m == INV ? ((uint64_t)v << 32) : (((uint64_t)(m ^ 1u) << 32) | 1ull);
}

__global__ void k_jump(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t n2, uint32_t* changed) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2) return;
  const uint64_t a = in[v];
  const uint32_t p = (uint32_t)(a >> 32);
  const uint64_t b = in[p];
  const uint32_t pp = (uint32_t)(b >> 32);
  if (pp != p) {  // p is not a head yet: jump over it
    out[v] = ((uint64_t)pp << 32) | (uint32_t)((uint32_t)a + (uint32_t)b);
    *changed = 1u;
  } else {
    out[v] = a;
  }
}

// tails report the length of their chain to the head
__global__ void k_tail(const uint32_t* __restrict__ nxt, const uint64_t* __restrict__ pd, uint32_t n2,
                       uint32_t* __restrict__ len, uint32_t* __restrict__ tailof) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2 || nxt[v] != INV) return;
  const uint64_t a = pd[v];
  const uint32_t h = (uint32_t)(a >> 32);
  if ((uint32_t)(pd[h] >> 32) != h) return;  // on a cycle (cannot happen for a tail, kept for safety)
  len[h] = (uint32_t)a + 1u;
  tailof[h] = v;
}

// cnt[v] = length of the chain headed by v when that chain is the one kept of its mirrored pair.
// EVEN (even k): a k-mer that is a unitig of its own is numbered on the strand the host's walk starts on (dbg.cpp:
// unitig_order) — strand 1 when its strand-0 row is empty and strand 1 has an out-edge.  A palindromic k-mer is always
// such a unitig (no edge at it is internal), and its two rows are no mirror images: this fixes its flip.
template <bool EVEN>
__global__ void k_keep(const uint32_t* __restrict__ len, const uint32_t* __restrict__ tailof, uint32_t n2,
                       uint32_t* __restrict__ cnt, uint32_t* n_kept, const uint32_t* __restrict__ succ) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2) return;
  const uint32_t l = len[v];
  bool keep = l != 0u && v < (tailof[v] ^ 1u);
  if constexpr (EVEN) {
    if (l == 1u) {
      uint32_t deg0, deg1;
      (void)only_succ(succ, v & ~1u, &deg0);
      (void)only_succ(succ, v | 1u, &deg1);
      keep = (v & 1u) == ((deg0 == 0u && deg1 > 0u) ? 1u : 0u);
    }
  }
  cnt[v] = keep ? l : 0u;
  if (keep) atomicAdd(n_kept, 1u);
}

__global__ void k_assign(const uint64_t* __restrict__ pd, const uint32_t* __restrict__ cnt,
                         const uint32_t* __restrict__ base, uint32_t n2, uint32_t* __restrict__ rank2id,
                         uint8_t* __restrict__ flip) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n2) return;
  const uint64_t a = pd[v];
  const uint32_t h = (uint32_t)(a >> 32);
  if ((uint32_t)(pd[h] >> 32) != h || cnt[h] == 0u) return;  // cycle, or the mirrored chain is the kept one
  rank2id[v >> 1] = base[h] + (uint32_t)a;
  flip[v >> 1] = (uint8_t)(v & 1u);
}

// ---- successor (and, at even k, predecessor) table in sorted-rank space (dbg.cpp: build_tables_rank) -------------
typedef unsigned __int128 u128;
using g2s::u256;

__device__ __forceinline__ uint64_t d_revcomp32(uint64_t x) {  // all 32 bases of a word (kmer.hpp)
  x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
  x = __builtin_bswap64(x);
  return x ^ 0xAAAAAAAAAAAAAAAAULL;
}
__device__ __forceinline__ uint64_t d_revcomp(uint64_t x, int k) { return d_revcomp32(x) >> (64 - 2 * k); }
__device__ __forceinline__ u128 d_revcomp(u128 x, int k) {
  const u128 y = ((u128)d_revcomp32((uint64_t)x) << 64) | (u128)d_revcomp32((uint64_t)(x >> 64));
  return y >> (128 - 2 * k);
}
__device__ __forceinline__ u256 d_revcomp(const u256& x, int k) {
  const u128 h = ((u128)d_revcomp32(x.word(0)) << 64) | (u128)d_revcomp32(x.word(1));
  const u128 l = ((u128)d_revcomp32(x.word(2)) << 64) | (u128)d_revcomp32(x.word(3));
  return u256(h, l) >> (256 - 2 * k);
}

template <class KT>
__device__ __forceinline__ uint32_t d_rank_of(const KT* __restrict__ v, const uint32_t* __restrict__ bucket, int shift,
                                              KT x) {
  const uint32_t b = (uint32_t)(x >> shift);
  uint32_t lo = bucket[b], hi = bucket[b + 1];
  const uint32_t end = hi;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < end && v[lo] == x) ? lo : INV;
}

// EVEN (even k; dbg.cpp: build_tables_rank): a palindromic k-mer (c == revcomp(c)) exists on strand 1 only — its strand-0
// rows stay INVALID in both tables, and a neighbour that is a palindrome is named with orientation 1 (the tie rule).  The
// predecessor table comes from the same searches: the successor y of the oriented node t by nt is, read on the other
// strand, the predecessor by nt of the node whose sequence is t's reverse complement — t ^ 1, or t itself when t is a
// palindrome — with the orientation of the other strand, ties to 1 again.
template <bool EVEN>
__device__ __forceinline__ void d_store_rows(uint32_t t, bool pal, const uint32_t (&out)[4], const uint32_t (&pout)[4],
                                             uint32_t* __restrict__ succ, uint32_t* __restrict__ pred) {
  *(uint4*)(succ + (size_t)t * 4) = make_uint4(out[0], out[1], out[2], out[3]);
  if constexpr (EVEN) *(uint4*)(pred + (size_t)(pal ? t : (t ^ 1u)) * 4) = make_uint4(pout[0], pout[1], pout[2], pout[3]);
}

template <class KT, bool EVEN>
__global__ void k_succ(const KT* __restrict__ v, const uint32_t* __restrict__ bucket, int shift, uint32_t n2, int k,
                       uint32_t* __restrict__ succ, uint32_t* __restrict__ pred) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // oriented node in rank space: 2*rank + strand
  if (t >= n2) return;
  const KT mask = (2 * k >= (int)(8 * sizeof(KT))) ? ~(KT)0 : ((((KT)1) << (2 * k)) - 1);
  const KT c = v[t >> 1], rc = d_revcomp(c, k);
  const KT seq = (t & 1u) ? rc : c, rseq = (t & 1u) ? c : rc;
  const bool pal = EVEN && c == rc;
  uint32_t out[4] = {INV, INV, INV, INV}, pout[4] = {INV, INV, INV, INV};
  if (!(pal && (t & 1u) == 0u)) {
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const KT y = ((seq << 2) | (KT)nt) & mask;
      const KT ry = (rseq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));
      const uint32_t r = d_rank_of<KT>(v, bucket, shift, y < ry ? y : ry);
      out[nt] = r == INV ? INV : 2u * r + (y < ry ? 0u : 1u);
      if constexpr (EVEN) pout[nt] = r == INV ? INV : 2u * r + (ry < y ? 0u : 1u);
    }
  }
  d_store_rows<EVEN>(t, pal, out, pout, succ, pred);
}

// set graphs (dbg.cpp: graph_build_sets): the neighbour searched inside its own set's rank range only — sets are small,
// a binary search over the range replaces the prefix index over the union
template <class KT, bool EVEN>
__global__ void k_succ_set(const KT* __restrict__ v, const uint32_t* __restrict__ rank_set, const uint32_t* __restrict__ set_lo,
                           uint32_t n2, int k, uint32_t* __restrict__ succ, uint32_t* __restrict__ pred) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // oriented node in rank space: 2*rank + strand
  if (t >= n2) return;
  const KT mask = (2 * k >= (int)(8 * sizeof(KT))) ? ~(KT)0 : ((((KT)1) << (2 * k)) - 1);
  const KT c = v[t >> 1], rc = d_revcomp(c, k);
  const KT seq = (t & 1u) ? rc : c, rseq = (t & 1u) ? c : rc;
  const bool pal = EVEN && c == rc;
  const uint32_t set = rank_set[t >> 1], lo0 = set_lo[set], hi0 = set_lo[set + 1];
  uint32_t out[4] = {INV, INV, INV, INV}, pout[4] = {INV, INV, INV, INV};
  if (!(pal && (t & 1u) == 0u)) {
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const KT y = ((seq << 2) | (KT)nt) & mask;
      const KT ry = (rseq >> 2) | ((KT)(nt ^ 2) << (2 * (k - 1)));
      const KT x = y < ry ? y : ry;
      uint32_t lo = lo0, hi = hi0;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
      }
      const bool hit = lo < hi0 && v[lo] == x;
      out[nt] = hit ? 2u * lo + (y < ry ? 0u : 1u) : INV;
      if constexpr (EVEN) pout[nt] = hit ? 2u * lo + (ry < y ? 0u : 1u) : INV;
    }
  }
  d_store_rows<EVEN>(t, pal, out, pout, succ, pred);
}

// ---- tables in id space (dbg.cpp: finish_graph) ----------------------------------------------
template <class KT, bool EVEN>
__global__ void k_remap(const KT* __restrict__ v, const uint32_t* __restrict__ succ_r, const uint32_t* __restrict__ pred_r,
                        const uint32_t* __restrict__ rank2id, const uint8_t* __restrict__ flip, uint32_t n2, int k,
                        uint32_t* __restrict__ succ_id, uint32_t* __restrict__ pred_id, uint8_t* __restrict__ lastnt,
                        uint32_t* __restrict__ id2rank) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n2) return;
  const uint32_t r = t >> 1, s = t & 1u;
  const uint32_t row = 2u * rank2id[r] + (s ^ (uint32_t)flip[r]);
  const uint4 in = *(const uint4*)(succ_r + (size_t)t * 4);
  auto remap = [&](uint32_t w) -> uint32_t { return w == INV ? INV : 2u * rank2id[w >> 1] + ((w & 1u) ^ (uint32_t)flip[w >> 1]); };
  *(uint4*)(succ_id + (size_t)row * 4) = make_uint4(remap(in.x), remap(in.y), remap(in.z), remap(in.w));
  if constexpr (EVEN) {  // the explicit predecessor table (even k only)
    const uint4 pin = *(const uint4*)(pred_r + (size_t)t * 4);
    *(uint4*)(pred_id + (size_t)row * 4) = make_uint4(remap(pin.x), remap(pin.y), remap(pin.z), remap(pin.w));
  }
  const KT c = v[r];
  lastnt[row] = s == 0 ? (uint8_t)(c & 3) : (uint8_t)(((c >> (2 * (k - 1))) & 3) ^ 2);
  if (s == 0) id2rank[rank2id[r]] = r;
}

// unitig-start bitmap from the id-space table (dbg.cpp: build_ustart); one wave per 64-bit word
__global__ void k_ustart(const uint32_t* __restrict__ succ, uint32_t n, uint32_t nbits, uint64_t* __restrict__ words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool start = true;
  if (i < n && i > 0) {
    const uint32_t v = 2u * (i - 1u), want = 2u * i;
    uint32_t deg, w = only_succ(succ, v, &deg);
    if (deg == 1 && w == want) {
      uint32_t dback, back = only_succ(succ, want ^ 1u, &dback);
      start = !(dback == 1 && back == (v ^ 1u));
    }
  }
  const uint64_t m = __ballot(i < nbits && start);
  if ((threadIdx.x & 63u) == 0 && i < nbits) words[i >> 6] = m;
}

// ---- solid k-mer set (dbg.cpp: count_solid) ----------------------------------------------
// one thread per text position: the canonical k-mer starting there, or all-ones when the
// window holds an N/n (GATB: k-mers with an invalid character are skipped) or runs off the end
template <class KT>
__global__ void k_extract(const uint8_t* __restrict__ text, uint64_t len, int k, KT* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  KT f = 0;
  bool ok = i + (uint64_t)k <= len;
  if (ok) {
    for (int j = 0; j < k; j++) {
      const uint8_t c = text[i + (uint64_t)j];
      ok = ok && ((c >> 3) & 1u) == 0u;
      f = (f << 2) | (KT)((c >> 1) & 3u);
    }
  }
  const KT r = d_revcomp(f, k);
  keys[i] = ok ? (f < r ? f : r) : ~(KT)0;
}
template <class KT>
__global__ void k_split(const KT* __restrict__ keys, uint64_t n, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lo[i] = (uint64_t)keys[i];
  hi[i] = (uint64_t)(keys[i] >> 64);
}
__global__ void k_join(const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi, uint64_t n, u128* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = ((u128)hi[i] << 64) | (u128)lo[i];
}
// 256-bit keys are sorted as four stable 64-bit LSD passes over (word, index) pairs: before pass `w` the w-th word of
// every key in the order of the passes so far (word 0 in text order, idx == nullptr), after the last pass the keys
// gathered once (32-byte keys do not move four times)
__global__ void k_word(const u256* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n, int w,
                       uint64_t* __restrict__ word, uint32_t* __restrict__ iota) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* src = (const uint64_t*)(keys + (idx ? idx[i] : (uint32_t)i));  // (u256: little-endian words)
  word[i] = src[w];
  if (!idx) iota[i] = (uint32_t)i;
}
__global__ void k_gather(const u256* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n, u256* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = keys[idx[i]];
}
// heads of runs of equal keys in the sorted array (the all-ones filler is no k-mer)
template <class KT>
__global__ void k_heads(const KT* __restrict__ keys, uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KT x = keys[i];
  flag[i] = (x != ~(KT)0 && (i == 0 || keys[i - 1] != x)) ? 1u : 0u;
}
template <class KT>
__global__ void k_head_index(const KT* __restrict__ keys, const uint32_t* __restrict__ flag,
                             const uint32_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ hidx,
                             uint32_t* n_valid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) hidx[pos[i]] = (uint32_t)i;
  // the first filler (or the end) closes the last run
  if (keys[i] != ~(KT)0 && (i + 1 == n || keys[i + 1] == ~(KT)0)) *n_valid = (uint32_t)(i + 1);
}
__global__ void k_solid_flag(const uint32_t* __restrict__ hidx, uint32_t nheads, uint32_t n_valid, uint32_t solid,
                             uint32_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nheads) return;
  const uint32_t end = j + 1 < nheads ? hidx[j + 1] : n_valid;
  keep[j] = (end - hidx[j] >= solid) ? 1u : 0u;
}
template <class KT>
__global__ void k_compact(const KT* __restrict__ keys, const uint32_t* __restrict__ hidx, const uint32_t* __restrict__ keep,
                          const uint32_t* __restrict__ kpos, uint32_t nheads, KT* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nheads || !keep[j]) return;
  out[kpos[j]] = keys[hidx[j]];
}
// prefix index over the sorted set: bucket[b] = first rank whose top bits are >= b
template <class KT>
__global__ void k_bucket(const KT* __restrict__ v, uint32_t n, int shift, uint32_t nb, uint32_t* __restrict__ bucket) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)(v[mid] >> shift) < (uint64_t)b) lo = mid + 1; else hi = mid;
  }
  bucket[b] = lo;
}

// ---- keyed solid k-mer sets (set graphs): sort key (set, canonical k-mer), set most significant
// the set of every text position: seq_start[j] = where sequence j starts in the text (one separator after each)
__global__ void k_pos_set(const uint64_t* __restrict__ seq_start, const uint32_t* __restrict__ seq_set, uint32_t nseqs, uint64_t T,
                          uint32_t* __restrict__ sid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  uint32_t lo = 0, hi = nseqs;  // the last sequence starting at or before i
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seq_start[mid] <= i) lo = mid; else hi = mid;
  }
  sid[i] = seq_set[lo];
}
// word w (little-endian 64-bit words) of every key in the order of the passes so far (idx == nullptr: text order);
// w == -1: the key's set id
template <class KT>
__global__ void k_key_word(const KT* __restrict__ keys, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ idx, uint64_t n,
                           int w, uint64_t* __restrict__ word, uint32_t* __restrict__ iota) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx ? idx[i] : (uint32_t)i;
  word[i] = w < 0 ? (uint64_t)sid[j] : ((const uint64_t*)(keys + j))[w];
  if (!idx) iota[i] = (uint32_t)i;
}
template <class KT>
__global__ void k_gather_keyed(const KT* __restrict__ keys, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ idx,
                               uint64_t n, KT* __restrict__ out, uint32_t* __restrict__ out_sid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = keys[idx[i]];
  out_sid[i] = sid[idx[i]];
}
// run heads and tails over (set, k-mer); the all-ones filler (a window with an N, or over a separator) is no k-mer
template <class KT>
__global__ void k_heads_keyed(const KT* __restrict__ keys, const uint32_t* __restrict__ sid, uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KT x = keys[i];
  flag[i] = (x != ~(KT)0 && (i == 0 || keys[i - 1] != x || sid[i - 1] != sid[i])) ? 1u : 0u;
}
// run j = [hidx[j], tidx[j]]; (a position's run: the inclusive scan of the heads minus one)
template <class KT>
__global__ void k_runs_keyed(const KT* __restrict__ keys, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ flag,
                             const uint32_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ hidx, uint32_t* __restrict__ tidx) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const KT x = keys[i];
  if (x == ~(KT)0) return;
  const uint32_t run = pos[i] + flag[i] - 1u;
  if (flag[i]) hidx[run] = (uint32_t)i;
  if (i + 1 == n || keys[i + 1] != x || sid[i + 1] != sid[i]) tidx[run] = (uint32_t)i;
}
__global__ void k_solid_keyed(const uint32_t* __restrict__ hidx, const uint32_t* __restrict__ tidx, uint32_t nruns, uint32_t solid,
                              uint32_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nruns) return;
  keep[j] = (tidx[j] - hidx[j] + 1u >= solid) ? 1u : 0u;
}
template <class KT>
__global__ void k_compact_keyed(const KT* __restrict__ keys, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ hidx,
                                const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kpos, uint32_t nruns,
                                KT* __restrict__ out, uint32_t* __restrict__ out_sid) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nruns || !keep[j]) return;
  out[kpos[j]] = keys[hidx[j]];
  out_sid[kpos[j]] = sid[hidx[j]];
}
// every set's first rank in the set-major solid k-mer array (nsets + 1 entries, the last = n)
__global__ void k_set_first(const uint32_t* __restrict__ rank_set, uint32_t n, uint32_t nsets, uint32_t* __restrict__ set_lo) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nsets) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (rank_set[mid] < s) lo = mid + 1; else hi = mid;
  }
  set_lo[s] = lo;
}

// ---- pooled set graphs (dbg.hpp: PoolSets): the pool's k-mers are extracted once, one key per pool position; the sets'
// lists name pool sequences, an INSTANCE being one occurrence of a sequence in a list (own lists in set order, or
// the shared list)
__global__ void k_inst_len(const uint32_t* __restrict__ inst_seq, const uint32_t* __restrict__ seq_len1, uint32_t ninst,
                           uint32_t* __restrict__ len1) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < ninst) len1[j] = seq_len1[inst_seq[j]];
}
// The text of the sequences in use that lie in a device-held pool (dbg.hpp: PoolDeviceText), copied device to device to
// their places in the build's text, each with its separator.  A wave a read: reads are 50 to 250 bytes, so one step of
// 64 lanes x 4 bytes covers most of them, and a wave's loads and stores are each one run of consecutive dwords.  Source
// and destination are not mutually aligned: the destination is brought to a 4-byte boundary by bytes, every lane then
// stores one aligned dword made of the two aligned source dwords around its place (both hold a byte of the read, and
// the pool's text begins on a 256-byte boundary, so neither load leaves the pool's allocation); the tail of up to three
// bytes and the 'N' go by bytes.  A read whose place would end beyond the text is skipped (the host checked; belt and
// braces).
struct GatherSource {
  const uint8_t* text;
  const uint64_t* start;
};
__global__ void __launch_bounds__(256) k_gather_reads(const GatherSource* __restrict__ src, const uint32_t* __restrict__ g_src,
                                                      const uint32_t* __restrict__ g_read, const uint32_t* __restrict__ g_dst,
                                                      const uint32_t* __restrict__ g_len1, uint32_t n,
                                                      uint8_t* __restrict__ text, uint64_t P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + threadIdx.x / 64; i < n; i += waves) {
    const uint32_t len1 = g_len1[i];
    const uint64_t d0 = g_dst[i];
    if (len1 == 0 || d0 + len1 > P) continue;
    const uint32_t len = len1 - 1;
    const GatherSource S = src[g_src[i]];
    const uint8_t* from = S.text + S.start[g_read[i]];
    uint8_t* to = text + d0;  // (the text begins on a 256-byte boundary: d0 gives the alignment)
    const uint32_t head = min(len, (uint32_t)((4u - (uint32_t)(d0 & 3u)) & 3u));
    if (lane < head) to[lane] = from[lane];
    const uint32_t words = (len - head) / 4;
    const uint8_t* f = from + head;
    const uint32_t sh = (uint32_t)((uintptr_t)f & 3u);
    const uint32_t* fw = (const uint32_t*)(f - sh);
    uint32_t* tw = (uint32_t*)(to + head);
    for (uint32_t w = lane; w < words; w += 64) {
      uint32_t v = fw[w];
      if (sh) v = (v >> (8u * sh)) | (fw[w + 1] << (32u - 8u * sh));
      tw[w] = v;
    }
    const uint32_t done = head + 4 * words;
    if (lane < len - done) to[done + lane] = from[done + lane];
    if (lane == 0) to[len] = 'N';
  }
}
// one (key, set) pair per instance position: the instance by binary search in the instances' start table (the scan of
// their lengths + 1), the key by gather from the pool position.  A window that crosses the sequence's end or holds an
// N is the all-ones filler there already.  sid / inst_set == nullptr: keys only (the shared list).
template <class KT>
__global__ void k_pool_pairs(const KT* __restrict__ pool_keys, const uint32_t* __restrict__ inst_start,
                             const uint32_t* __restrict__ inst_seq, const uint32_t* __restrict__ inst_set,
                             const uint32_t* __restrict__ seq_start, uint32_t ninst, uint64_t I, KT* __restrict__ keys,
                             uint32_t* __restrict__ sid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  uint32_t lo = 0, hi = ninst;  // the last instance starting at or before i (every instance has a position: its separator)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)inst_start[mid] <= i) lo = mid; else hi = mid;
  }
  keys[i] = pool_keys[(size_t)seq_start[inst_seq[lo]] + (size_t)(i - inst_start[lo])];
  if (sid) sid[i] = inst_set[lo];
}
template <class KT>
__global__ void k_gather_keys(const KT* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n, KT* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = keys[idx[i]];
}
// the own lists' runs as a table: (k-mer, set, count), ascending by (set, k-mer)
template <class KT>
__global__ void k_run_table(const KT* __restrict__ sk, const uint32_t* __restrict__ ss, const uint32_t* __restrict__ hidx,
                            const uint32_t* __restrict__ tidx, uint32_t nruns, KT* __restrict__ rkey, uint32_t* __restrict__ rset,
                            uint32_t* __restrict__ rcnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nruns) return;
  rkey[j] = sk[hidx[j]];
  rset[j] = ss[hidx[j]];
  rcnt[j] = tidx[j] - hidx[j] + 1u;
}
// the shared list's runs as a table: (k-mer, count), ascending
template <class KT>
__global__ void k_shared_table(const KT* __restrict__ sorted, const uint32_t* __restrict__ hidx, uint32_t nheads, uint32_t n_valid,
                               KT* __restrict__ hkey, uint32_t* __restrict__ hcnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nheads) return;
  hkey[j] = sorted[hidx[j]];
  hcnt[j] = (j + 1 < nheads ? hidx[j + 1] : n_valid) - hidx[j];
}
template <class KT>
__device__ __forceinline__ uint32_t d_lower_bound(const KT* __restrict__ v, uint32_t lo, uint32_t hi, const KT& x) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// The merge of the own runs and the shared table, per set.  A set without the flag keeps its runs of at least `solid`
// copies.  A flagged set (set_fidx[s] = its number among the F flagged sets, else INV) keeps every shared k-mer whose
// shared count plus own count reaches `solid` (item f * U + u below) and every run of at least `solid` copies whose
// k-mer the shared table does not hold.  Both flag arrays carry one more entry, zero, so that their exclusive scans
// end in the totals.
template <class KT>
__global__ void k_pool_keep_own(const KT* __restrict__ rkey, const uint32_t* __restrict__ rset, const uint32_t* __restrict__ rcnt,
                                uint32_t nruns, const uint32_t* __restrict__ set_fidx, const KT* __restrict__ hkey, uint32_t U,
                                uint32_t solid, uint32_t* __restrict__ keep) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > nruns) return;
  bool kp = j < nruns && rcnt[j] >= solid;
  if (kp && set_fidx[rset[j]] != INV) {
    const KT x = rkey[j];
    const uint32_t u = d_lower_bound<KT>(hkey, 0u, U, x);
    kp = !(u < U && hkey[u] == x);  // (in the shared table: the shared item decides, on the sum)
  }
  keep[j] = kp ? 1u : 0u;
}
template <class KT>
__global__ void k_pool_keep_shared(const KT* __restrict__ hkey, const uint32_t* __restrict__ hcnt, uint32_t U,
                                   const uint32_t* __restrict__ fset, uint32_t FU, const uint32_t* __restrict__ run_lo,
                                   const KT* __restrict__ rkey, const uint32_t* __restrict__ rcnt, uint32_t solid,
                                   uint32_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > FU) return;
  if (i == FU) { keep[i] = 0u; return; }
  const uint32_t f = i / U, u = i - f * U, s = fset[f], hi = run_lo[s + 1];
  const KT x = hkey[u];
  const uint32_t r = d_lower_bound<KT>(rkey, run_lo[s], hi, x);
  const uint64_t own = (r < hi && rkey[r] == x) ? rcnt[r] : 0u;
  keep[i] = ((uint64_t)hcnt[u] + own >= (uint64_t)solid) ? 1u : 0u;
}
// every set's k-mers kept (pown / psh: the exclusive scans of the two flag arrays); cnt[nsets] = 0
__global__ void k_pool_set_count(const uint32_t* __restrict__ run_lo, const uint32_t* __restrict__ pown,
                                 const uint32_t* __restrict__ set_fidx, const uint32_t* __restrict__ psh, uint32_t U, uint32_t nsets,
                                 uint32_t* __restrict__ cnt) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nsets) return;
  uint32_t c = 0;
  if (s < nsets) {
    c = pown[run_lo[s + 1]] - pown[run_lo[s]];
    const uint32_t f = set_fidx[s];
    if (f != INV) c += psh[(f + 1u) * U] - psh[f * U];
  }
  cnt[s] = c;
}
// The output is written in (set, k-mer) order without a second sort: in set s, from base[s] on, a kept k-mer lands
// behind the kept shared k-mers and the kept own-only runs that are smaller than it.
template <class KT>
__global__ void k_pool_write_own(const KT* __restrict__ rkey, const uint32_t* __restrict__ rset, uint32_t nruns,
                                 const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pown,
                                 const uint32_t* __restrict__ run_lo, const uint32_t* __restrict__ set_fidx,
                                 const KT* __restrict__ hkey, uint32_t U, const uint32_t* __restrict__ psh,
                                 const uint32_t* __restrict__ base, KT* __restrict__ out, uint32_t* __restrict__ out_sid) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nruns || !keep[j]) return;
  const uint32_t s = rset[j], f = set_fidx[s];
  const KT x = rkey[j];
  uint32_t pos = base[s] + (pown[j] - pown[run_lo[s]]);
  if (f != INV) pos += psh[f * U + d_lower_bound<KT>(hkey, 0u, U, x)] - psh[f * U];
  out[pos] = x;
  out_sid[pos] = s;
}
template <class KT>
__global__ void k_pool_write_shared(const KT* __restrict__ hkey, uint32_t U, const uint32_t* __restrict__ fset, uint32_t FU,
                                    const uint32_t* __restrict__ keep, const uint32_t* __restrict__ psh,
                                    const uint32_t* __restrict__ run_lo, const KT* __restrict__ rkey,
                                    const uint32_t* __restrict__ pown, const uint32_t* __restrict__ base, KT* __restrict__ out,
                                    uint32_t* __restrict__ out_sid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= FU || !keep[i]) return;
  const uint32_t f = i / U, u = i - f * U, s = fset[f], lo = run_lo[s];
  const KT x = hkey[u];
  const uint32_t r = d_lower_bound<KT>(rkey, lo, run_lo[s + 1], x);  // (a run of x itself is not kept as own: either bound will do)
  const uint32_t pos = base[s] + (psh[i] - psh[f * U]) + (pown[r] - pown[lo]);
  out[pos] = x;
  out_sid[pos] = s;
}

// ---- reach sets of a pooled build (dbg.hpp: PoolReach): the k-mers of a set within `radius` undirected steps of its
// seeds, by a breadth-first search over the IMPLICIT full graph — a k-mer is in set s when its copies in the set's own
// runs plus, for a flagged set, in the shared table reach `solid`: two binary searches, as in k_pool_keep_shared /
// k_pool_keep_own.  Persistent workgroups draw sets from a ticket (one atomic add a claim); a set is searched by one
// workgroup from its seeds to its last level, so levels are separated by workgroup barriers only and no workgroup
// waits for another.  lane = (frontier k-mer, neighbour): 32 k-mers a step.  A k-mer is claimed by atomicOr on its
// bit — one bit per own run, one per (flagged set with a record, shared entry); the shared bit names a k-mer that is in
// both tables.  Claimed k-mers are staged in LDS and leave for the queue in device memory in chunks (one atomic add on
// the queue's fill a chunk); a level's chunks are the next level's frontier, read back from the queue, and the queue
// at the end holds every kept (k-mer, set) once.  Nothing is written past a buffer: a chunk that would not fit the
// queue, or the chunk list of a level, raises the overflow word instead and the search stops at the next ticket.
constexpr uint32_t kReachThreads = 256;
constexpr uint32_t kReachStage = 1024;   // k-mers staged in LDS before they leave as one chunk
constexpr uint32_t kReachChunks = 512;   // chunks of one level of one set
struct ReachArgs {
  const uint32_t* rsets;    // [R] the sets with a record
  const int32_t* radius;    // [R]
  const uint32_t* seed_lo;  // [R + 1] into the seeds
  const uint32_t* set_fr;   // [nsets] the set's row in the shared bitmap (flagged, with a record), else INV
  const uint32_t* run_lo;   // [nsets + 1]
  const uint32_t* rcnt;     // [nruns]
  const uint32_t* hcnt;     // [U]
  uint32_t* own_bits;       // [(nruns + 31) / 32]
  uint32_t* sh_bits;        // [rows * W]
  uint32_t* out_set;        // [Q]
  uint32_t* ctl;            // ticket, queue fill, overflow, deepest level
  uint32_t U, W, R, Q, solid;
  int k;
};
enum { kReachTicket = 0, kReachFill = 1, kReachOverflow = 2, kReachLevels = 3 };
enum : uint32_t { kReachQueueFull = 1u, kReachChunkListFull = 2u };  // bits of the overflow word

template <class KT>
__device__ __forceinline__ bool d_reach_claim(const ReachArgs& a, const KT* __restrict__ rkey, const KT* __restrict__ hkey, uint32_t s,
                                              uint32_t fr, const KT& x) {
  uint64_t cnt = 0;
  uint32_t u = 0;
  bool in_sh = false;
  if (fr != INV) {
    u = d_lower_bound<KT>(hkey, 0u, a.U, x);
    in_sh = u < a.U && hkey[u] == x;
    if (in_sh) cnt = a.hcnt[u];
  }
  const uint32_t hi = a.run_lo[s + 1], r = d_lower_bound<KT>(rkey, a.run_lo[s], hi, x);
  const bool in_own = r < hi && rkey[r] == x;
  if (in_own) cnt += a.rcnt[r];
  if ((!in_sh && !in_own) || cnt < (uint64_t)a.solid) return false;
  uint32_t* word = in_sh ? a.sh_bits + (size_t)fr * a.W + (u >> 5) : a.own_bits + (r >> 5);
  const uint32_t bit = 1u << ((in_sh ? u : r) & 31u);
  return (atomicOr(word, bit) & bit) == 0u;
}

template <class KT>
__global__ __launch_bounds__(256) void k_reach_bfs(ReachArgs a, const KT* __restrict__ rkey, const KT* __restrict__ hkey,
                                                   const KT* __restrict__ seeds, KT* __restrict__ out_key) {
  __shared__ __attribute__((aligned(16))) uint64_t stage_words[kReachStage * (sizeof(KT) / 8)];  // (u256 has constructors)
  KT* stage = (KT*)stage_words;
  __shared__ uint2 chunks[2][kReachChunks];
  __shared__ uint32_t n_stage, n_chunk[2], sh_r, sh_stop, sh_base;
  const uint32_t tid = threadIdx.x;
  const int k = a.k;
  const KT mask = (2 * k >= (int)(8 * sizeof(KT))) ? ~(KT)0 : ((((KT)1) << (2 * k)) - 1);
  for (;;) {
    __syncthreads();  // (the last set's reads of the words below are over)
    if (tid == 0) {
      sh_stop = atomicAdd(&a.ctl[kReachOverflow], 0u);
      sh_r = atomicAdd(&a.ctl[kReachTicket], 1u);
      n_stage = 0u;
      n_chunk[0] = 0u;
      n_chunk[1] = 0u;
    }
    __syncthreads();
    const uint32_t r = sh_r;
    if (r >= a.R || sh_stop) return;
    const uint32_t s = a.rsets[r], fr = a.set_fr[s];
    const uint32_t radius = (uint32_t)a.radius[r];
    // the staged k-mers leave as one chunk of level list `list`; false: no room (the overflow word is up)
    auto flush = [&](uint32_t list) -> bool {
      __syncthreads();
      const uint32_t n = n_stage;
      __syncthreads();
      if (n == 0u) return true;
      if (tid == 0) {
        const uint32_t base = atomicAdd(&a.ctl[kReachFill], n);
        // (after an overflow other workgroups may add to the fill once more each before they see the word at their next
        // ticket; should the 32-bit fill ever wrap, a later chunk lands inside the queue again — in bounds, and the
        // overflow word stays up, so the host discards all of it)
        const bool fits = (uint64_t)base + n <= (uint64_t)a.Q, listed = n_chunk[list] < kReachChunks;
        const bool ok = fits && listed;
        if (ok) chunks[list][n_chunk[list]++] = make_uint2(base, n);
        else atomicOr(&a.ctl[kReachOverflow], fits ? kReachChunkListFull : kReachQueueFull);
        sh_base = ok ? base : INV;
        n_stage = 0u;
      }
      __syncthreads();
      const uint32_t base = sh_base;
      if (base == INV) return false;
      for (uint32_t i = tid; i < n; i += kReachThreads) {
        out_key[(size_t)base + i] = stage[i];
        a.out_set[(size_t)base + i] = s;
      }
      __threadfence_block();
      __syncthreads();
      return true;
    };
    // room for one step's claims (at most one a lane) before the step
    auto room = [&](uint32_t list) -> bool {
      __syncthreads();
      const uint32_t n = n_stage;
      __syncthreads();
      return n + kReachThreads <= kReachStage ? true : flush(list);
    };
    bool ok = true;
    // level 0: the seeds that are k-mers of the set
    const uint32_t s_lo = a.seed_lo[r], s_hi = a.seed_lo[r + 1];
    for (uint32_t i0 = s_lo; ok && i0 < s_hi; i0 += kReachThreads) {
      ok = room(0u);
      if (!ok) break;
      if (i0 + tid < s_hi) {
        const KT x = seeds[i0 + tid];
        if (d_reach_claim<KT>(a, rkey, hkey, s, fr, x)) stage[atomicAdd(&n_stage, 1u)] = x;
      }
    }
    ok = ok && flush(0u);
    uint32_t cur = 0u, level = 0u;
    while (ok && n_chunk[cur] > 0u && level < radius) {
      const uint32_t nxt = cur ^ 1u, nc = n_chunk[cur];
      __syncthreads();
      if (tid == 0) n_chunk[nxt] = 0u;
      for (uint32_t c = 0; ok && c < nc; c++) {
        const uint2 ch = chunks[cur][c];
        for (uint32_t i0 = 0; i0 < ch.y; i0 += kReachThreads / 8u) {
          ok = room(nxt);
          if (!ok) break;
          const uint32_t item = i0 + (tid >> 3);
          if (item < ch.y) {
            const KT km = out_key[(size_t)ch.x + item], rc = d_revcomp(km, k);
            const uint32_t strand = (tid >> 2) & 1u, nt = tid & 3u;
            const KT seq = strand ? rc : km, rseq = strand ? km : rc;
            const KT y = ((seq << 2) | (KT)nt) & mask;
            const KT ry = (rseq >> 2) | ((KT)(nt ^ 2u) << (2 * (k - 1)));
            const KT x = y < ry ? y : ry;
            if (d_reach_claim<KT>(a, rkey, hkey, s, fr, x)) stage[atomicAdd(&n_stage, 1u)] = x;
          }
        }
      }
      ok = ok && flush(nxt);
      if (!ok || n_chunk[nxt] == 0u) break;
      level++;
      cur = nxt;
    }
    if (ok && tid == 0) atomicMax(&a.ctl[kReachLevels], level);
  }
}
// the run table with the sets with a record replaced by what their searches kept: every set's new run count ...
__global__ void k_reach_set_count(const uint32_t* __restrict__ run_lo, const uint32_t* __restrict__ set_ridx,
                                  const uint32_t* __restrict__ vis_lo, uint32_t nsets, uint32_t* __restrict__ cnt) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nsets) return;
  cnt[s] = s == nsets ? 0u : set_ridx[s] != INV ? vis_lo[s + 1] - vis_lo[s] : run_lo[s + 1] - run_lo[s];
}
// ... the runs of the sets without a record, copied ...
template <class KT>
__global__ void k_reach_copy_runs(const KT* __restrict__ rkey, const uint32_t* __restrict__ rset, const uint32_t* __restrict__ rcnt,
                                  uint32_t nruns, const uint32_t* __restrict__ set_ridx, const uint32_t* __restrict__ run_lo,
                                  const uint32_t* __restrict__ new_lo, KT* __restrict__ nkey, uint32_t* __restrict__ nset,
                                  uint32_t* __restrict__ ncnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nruns) return;
  const uint32_t s = rset[j];
  if (set_ridx[s] != INV) return;
  const uint32_t d = new_lo[s] + (j - run_lo[s]);
  nkey[d] = rkey[j];
  nset[d] = s;
  ncnt[d] = rcnt[j];
}
// ... and the kept k-mers (sorted by (set, k-mer)) as runs of `solid` copies: the merge keeps them as they are
template <class KT>
__global__ void k_reach_copy_kept(const KT* __restrict__ sk, const uint32_t* __restrict__ ss, uint32_t n,
                                  const uint32_t* __restrict__ vis_lo, const uint32_t* __restrict__ new_lo, uint32_t solid,
                                  KT* __restrict__ nkey, uint32_t* __restrict__ nset, uint32_t* __restrict__ ncnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = ss[i], d = new_lo[s] + (i - vis_lo[s]);
  nkey[d] = sk[i];
  nset[d] = s;
  ncnt[d] = solid;
}

}  // namespace

#include "graph_reach.h"

namespace g2s {

// Everything of the graph build after the sorted solid k-mer set (and its prefix index):
// successor table, unitig-ordered numbering, tables in id space, last-base table, unitig-start
// bitmap.  The id-space table and the bitmap stay on the device as the graph's copy for the
// fill path (g2s_graph_upload finds them).  `host_walk` numbers what list ranking leaves
// unnumbered (circular unitigs).  Returns false (with a reason) when the device cannot be
// used; nothing of g is touched then and the caller runs the host build.
template <class KT, bool EVEN>
static bool finish_gpu_e(Graph& g, int device, const std::function<void(const std::vector<uint32_t>&, uint32_t)>& host_walk,
                         std::string* why, const std::vector<uint32_t>* rank_set) {
  const std::vector<KT>& kmers = kmer_vec<KT>(g);
  if (!device_exists(device)) { if (why) *why = "no device"; return false; }
  const uint64_t n = g.n;
  if (n == 0 || 2 * n >= (1ull << 31)) { if (why) *why = "size"; return false; }
  G2S_HIP_TRY(hipSetDevice(device));
  const uint32_t n2 = (uint32_t)(2 * n);
  const int k = g.k;
  const dim3 blk(256), grd((n2 + 255) / 256);
  DevMem d_km, d_bucket, d_succ, d_pred, d_nxt, d_pd0, d_pd1, d_len, d_tail, d_cnt, d_base, d_id, d_flip, d_flag;
  Scratch d_tmp;
  // ---- successor table, rank space (even k: the predecessor table beside it; odd k allocates and writes none)
  G2S_HIP_TRY(d_km.alloc(kmers.size() * sizeof(KT)));
  G2S_HIP_TRY(d_succ.alloc((size_t)n2 * 16));
  if constexpr (EVEN) G2S_HIP_TRY(d_pred.alloc((size_t)n2 * 16));
  G2S_HIP_TRY(hipMemcpy(d_km.p, kmers.data(), kmers.size() * sizeof(KT), hipMemcpyHostToDevice));
  if (rank_set) {  // set graph: every neighbour searched in its own set's range (g.set_lo)
    DevMem d_rs, d_sl;
    std::vector<uint32_t> lo32(g.set_lo.begin(), g.set_lo.end());
    G2S_HIP_TRY(d_rs.alloc((size_t)n * 4));
    G2S_HIP_TRY(d_sl.alloc(lo32.size() * 4));
    G2S_HIP_TRY(hipMemcpy(d_rs.p, rank_set->data(), (size_t)n * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_sl.p, lo32.data(), lo32.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_succ_set<KT, EVEN>), grd, blk, 0, 0, (const KT*)d_km.p, (const uint32_t*)d_rs.p, (const uint32_t*)d_sl.p, n2,
                       k, (uint32_t*)d_succ.p, (uint32_t*)d_pred.p);
    G2S_HIP_TRY(hipDeviceSynchronize());
  } else {
    G2S_HIP_TRY(d_bucket.alloc(g.bucket.size() * 4));
    G2S_HIP_TRY(hipMemcpy(d_bucket.p, g.bucket.data(), g.bucket.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_succ<KT, EVEN>), grd, blk, 0, 0, (const KT*)d_km.p, (const uint32_t*)d_bucket.p, 2 * k - g.bucket_bits, n2,
                       k, (uint32_t*)d_succ.p, (uint32_t*)d_pred.p);
  }
  // ---- numbering along unitigs: list ranking
  G2S_HIP_TRY(d_nxt.alloc((size_t)n2 * 4));
  G2S_HIP_TRY(d_pd0.alloc((size_t)n2 * 8));
  G2S_HIP_TRY(d_pd1.alloc((size_t)n2 * 8));
  G2S_HIP_TRY(d_len.alloc((size_t)n2 * 4));
  G2S_HIP_TRY(d_tail.alloc((size_t)n2 * 4));
  G2S_HIP_TRY(d_cnt.alloc((size_t)n2 * 4));
  G2S_HIP_TRY(d_base.alloc((size_t)n2 * 4));
  G2S_HIP_TRY(d_id.alloc((size_t)n * 4));
  G2S_HIP_TRY(d_flip.alloc((size_t)n));
  G2S_HIP_TRY(d_flag.alloc(16));
  G2S_HIP_TRY(hipMemset(d_len.p, 0, (size_t)n2 * 4));
  G2S_HIP_TRY(hipMemset(d_tail.p, 0, (size_t)n2 * 4));
  G2S_HIP_TRY(hipMemset(d_id.p, 0xFF, (size_t)n * 4));
  G2S_HIP_TRY(hipMemset(d_flip.p, 0, (size_t)n));
  hipLaunchKernelGGL(k_next, grd, blk, 0, 0, (const uint32_t*)d_succ.p, n2, (uint32_t*)d_nxt.p);
  hipLaunchKernelGGL(k_init, grd, blk, 0, 0, (const uint32_t*)d_nxt.p, n2, (uint64_t*)d_pd0.p);
  uint64_t *cur = (uint64_t*)d_pd0.p, *oth = (uint64_t*)d_pd1.p;
  for (int round = 0; round < 34; round++) {  // 2^32 > any chain; cycles never settle and stop here
    G2S_HIP_TRY(hipMemset(d_flag.p, 0, 4));
    hipLaunchKernelGGL(k_jump, grd, blk, 0, 0, (const uint64_t*)cur, oth, n2, (uint32_t*)d_flag.p);
    uint32_t changed = 0;
    G2S_HIP_TRY(hipMemcpy(&changed, d_flag.p, 4, hipMemcpyDeviceToHost));
    std::swap(cur, oth);
    if (!changed) break;
  }
  hipLaunchKernelGGL(k_tail, grd, blk, 0, 0, (const uint32_t*)d_nxt.p, (const uint64_t*)cur, n2, (uint32_t*)d_len.p,
                     (uint32_t*)d_tail.p);
  G2S_HIP_TRY(hipMemset(d_flag.p, 0, 4));
  hipLaunchKernelGGL(k_keep<EVEN>, grd, blk, 0, 0, (const uint32_t*)d_len.p, (const uint32_t*)d_tail.p, n2, (uint32_t*)d_cnt.p,
                     (uint32_t*)d_flag.p, (const uint32_t*)d_succ.p);
  G2S_HIP_TRY(exclusive_scan(d_tmp, (const uint32_t*)d_cnt.p, (uint32_t*)d_base.p, (size_t)n2));
  hipLaunchKernelGGL(k_assign, grd, blk, 0, 0, (const uint64_t*)cur, (const uint32_t*)d_cnt.p, (const uint32_t*)d_base.p, n2,
                     (uint32_t*)d_id.p, (uint8_t*)d_flip.p);
  G2S_HIP_TRY(hipGetLastError());
  uint32_t kept = 0, next_id = 0;  // next_id: the ids handed out so far
  G2S_HIP_TRY(hipMemcpy(&kept, d_flag.p, 4, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(read_total((const uint32_t*)d_cnt.p, (const uint32_t*)d_base.p, (size_t)n2, &next_id));
  // free the ranking scratch before the id-space tables are allocated
  d_nxt.free(); d_pd0.free(); d_pd1.free(); d_len.free(); d_tail.free(); d_cnt.free(); d_base.free(); d_tmp.free();
  // ---- everything that can still fail is done: from here on g is written
  g.rank2id.assign((size_t)n, kInvalidNode);
  g.flip.assign((size_t)n, 0);
  g.n_unitigs = kept;
  if (next_id < n) {  // circular unitigs: the host walk numbers them after the rest
    std::vector<uint32_t> succ_r((size_t)n2 * 4);
    G2S_HIP_TRY(hipMemcpy(succ_r.data(), d_succ.p, (size_t)n2 * 16, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(g.rank2id.data(), d_id.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(g.flip.data(), d_flip.p, (size_t)n, hipMemcpyDeviceToHost));
    host_walk(succ_r, next_id);
    if (rank_set) {
      // Set graphs: the walk numbered the circular unitigs after every set; each moves to the end of its own set's
      // range (a stable reorder of the ids by set: list ranking's ids are set-major already — a chain's head and its
      // nodes are in one set, heads take ids in rank order)
      std::vector<uint32_t> id_set((size_t)n);
      for (uint64_t r = 0; r < n; r++) id_set[g.rank2id[(size_t)r]] = (*rank_set)[(size_t)r];
      std::vector<uint32_t> fill(g.set_lo.begin(), g.set_lo.end() - 1), new_id((size_t)n);
      for (uint64_t id = 0; id < n; id++) new_id[(size_t)id] = fill[id_set[(size_t)id]]++;
      for (uint64_t r = 0; r < n; r++) g.rank2id[(size_t)r] = new_id[g.rank2id[(size_t)r]];
    }
    G2S_HIP_TRY(hipMemcpy(d_id.p, g.rank2id.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_flip.p, g.flip.data(), (size_t)n, hipMemcpyHostToDevice));
  }
  // ---- tables in id space
  DevMem d_sid, d_pid, d_last, d_i2r, d_us;
  const size_t sbytes = (size_t)n2 * 16;
  if constexpr (EVEN) G2S_HIP_TRY(d_pid.alloc(sbytes));
  const size_t words = (size_t)((n + 63) / 64 + 1);
  G2S_HIP_TRY(d_sid.alloc(sbytes + 1024));  // INVALID padding behind the table, as the host build's upload has it
  G2S_HIP_TRY(hipMemset(d_sid.p, 0xFF, sbytes + 1024));
  G2S_HIP_TRY(d_last.alloc((size_t)n2));
  G2S_HIP_TRY(d_i2r.alloc((size_t)n * 4));
  G2S_HIP_TRY(d_us.alloc((words + 2 * kUstartPad) * 8));
  G2S_HIP_TRY(hipMemset(d_us.p, 0xFF, (words + 2 * kUstartPad) * 8));
  hipLaunchKernelGGL((k_remap<KT, EVEN>), grd, blk, 0, 0, (const KT*)d_km.p, (const uint32_t*)d_succ.p, (const uint32_t*)d_pred.p,
                     (const uint32_t*)d_id.p, (const uint8_t*)d_flip.p, n2, k, (uint32_t*)d_sid.p, (uint32_t*)d_pid.p,
                     (uint8_t*)d_last.p, (uint32_t*)d_i2r.p);
  const uint32_t nbits = (uint32_t)(words * 64);
  hipLaunchKernelGGL(k_ustart, dim3((nbits + 255) / 256), blk, 0, 0, (const uint32_t*)d_sid.p, (uint32_t)n, nbits,
                     (uint64_t*)d_us.p + kUstartPad);
  G2S_HIP_TRY(hipGetLastError());
  g.succ.resize((size_t)n2 * 4);
  g.pred.clear();
  if constexpr (EVEN) g.pred.resize((size_t)n2 * 4);
  g.lastnt.resize((size_t)n2);
  g.id2rank.resize((size_t)n);
  g.ustart.resize(words);
  G2S_HIP_TRY(hipMemcpy(g.succ.data(), d_sid.p, sbytes, hipMemcpyDeviceToHost));
  if constexpr (EVEN) G2S_HIP_TRY(hipMemcpy(g.pred.data(), d_pid.p, sbytes, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(g.lastnt.data(), d_last.p, (size_t)n2, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(g.id2rank.data(), d_i2r.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(g.ustart.data(), (uint64_t*)d_us.p + kUstartPad, words * 8, hipMemcpyDeviceToHost));
  if (next_id >= n) {
    G2S_HIP_TRY(hipMemcpy(g.rank2id.data(), d_id.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(g.flip.data(), d_flip.p, (size_t)n, hipMemcpyDeviceToHost));
  }
  // the device copy of the graph for the fill path
  DeviceGraph dg;
  dg.succ = (uint32_t*)d_sid.release();
  dg.ustart = (uint64_t*)d_us.release() + kUstartPad;
  dg.bytes = sbytes + (words + 2 * kUstartPad) * 8;
  if constexpr (EVEN) {
    dg.pred = (uint32_t*)d_pid.release();
    dg.bytes += sbytes;
  }
  g.dev[device] = dg;
  return true;
}

template <class KT>
static bool finish_gpu_t(Graph& g, int device, const std::function<void(const std::vector<uint32_t>&, uint32_t)>& host_walk,
                         std::string* why, const std::vector<uint32_t>* rank_set = nullptr) {
  return (g.k % 2) == 0 ? finish_gpu_e<KT, true>(g, device, host_walk, why, rank_set)
                        : finish_gpu_e<KT, false>(g, device, host_walk, why, rank_set);
}

// solid_passes.h
template <class KT>
static bool count_solid_passes_gpu_t(Graph& g, std::vector<KT>& out, const BuildInput& in, int solid, uint64_t T, double per_key,
                                     std::string* why, SolidCountInfo* info);
static bool solid_passes_forced();

// The sorted set of solid canonical k-mers and its prefix index, from the reads.  One key per
// text position, radix sort (rocPRIM; 128-bit keys as two stable 64-bit passes, 256-bit keys as four over
// (word, index) pairs), run heads,
// runs of at least `solid` copies compacted.  A text beyond one sort (2^32 positions, or half the free memory at the
// sort's bytes a position) goes through the key-range passes of solid_passes.h, as does every text under
// G2S_BUILD_PASS_KEYS.  Returns false (g untouched) when the device cannot be used or not even the passes fit.
template <class KT>
static bool count_solid_gpu_t(Graph& g, const BuildInput& in, int solid, int device, std::string* why, SolidCountInfo* info) {
  std::vector<KT>& out = kmer_vec<KT>(g);
  if (in.text) device = in.text->device;  // (where the text is)
  if (!device_exists(device)) { if (why) *why = "no device"; return false; }
  G2S_HIP_TRY(hipSetDevice(device));
  const int k = g.k;
  uint64_t T = 0;
  if (in.text) T = in.text->T;
  else for (auto& sq : *in.seqs) T += sq.second + 1;  // one separator after every sequence
  if (T == 0) { if (why) *why = "text size"; return false; }
  size_t free_b = 0, total_b = 0;
  G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  // (bytes a text position at the sort's peak: keys, sorted copy or split words, the sort's scratch; 256-bit keys:
  // the keys, the word and index double buffers, the sort's scratch, then the keys and their gathered copy)
  const double per_pos = sizeof(KT) == 32 ? (double)(2 * sizeof(KT) + 40) : (double)(4 * sizeof(KT) + 24);
  if (T >= (1ull << 32) || (double)T * per_pos > 0.5 * (double)free_b || solid_passes_forced())
    return count_solid_passes_gpu_t<KT>(g, out, in, solid, T, per_pos, why, info);
  DevMem d_text, d_keys, d_alt, d_lo, d_hi, d_lo2, d_hi2, d_flag, d_pos, d_hidx, d_keep, d_kpos, d_out;
  Scratch d_tmp;
  DevMem d_misc;
  if (!in.text) {
    std::vector<uint8_t> text((size_t)T);
    size_t pos = 0;
    for (auto& sq : *in.seqs) { memcpy(text.data() + pos, sq.first, (size_t)sq.second); pos += (size_t)sq.second; text[pos++] = 'N'; }
    G2S_HIP_TRY(d_text.alloc((size_t)T));
    G2S_HIP_TRY(hipMemcpy(d_text.p, text.data(), (size_t)T, hipMemcpyHostToDevice));
  }
  G2S_HIP_TRY(d_keys.alloc((size_t)T * sizeof(KT)));
  G2S_HIP_TRY(d_misc.alloc(16));
  const dim3 blk(256), grdT((unsigned)((T + 255) / 256));
  hipLaunchKernelGGL(k_extract<KT>, grdT, blk, 0, 0, in.text ? (const uint8_t*)in.text->d_text : (const uint8_t*)d_text.p, T, k,
                     (KT*)d_keys.p);
  if (in.text) free_device_text(in.text);  // (as d_text.free(): the text is not needed beside the sort)
  d_text.free();
  KT* sorted = nullptr;
  if constexpr (sizeof(KT) == 8) {
    G2S_HIP_TRY(d_alt.alloc((size_t)T * 8));
    // (the filler is all-ones: sort on all 64 bits so that it ends up last)
    G2S_HIP_TRY(radix_sort_keys(d_tmp, (uint64_t*)d_keys.p, (uint64_t*)d_alt.p, (size_t)T));
    sorted = (KT*)d_alt.p;
  } else if constexpr (sizeof(KT) == 32) {
    G2S_HIP_TRY(d_lo.alloc((size_t)T * 8));   // the pass's word, in and out
    G2S_HIP_TRY(d_lo2.alloc((size_t)T * 8));
    G2S_HIP_TRY(d_hi.alloc((size_t)T * 4));   // the key's index, in and out
    G2S_HIP_TRY(d_hi2.alloc((size_t)T * 4));
    uint64_t *w_in = (uint64_t*)d_lo.p, *w_out = (uint64_t*)d_lo2.p;
    uint32_t *i_in = (uint32_t*)d_hi.p, *i_out = (uint32_t*)d_hi2.p;
    G2S_HIP_TRY((radix_sort_pairs_reserve<uint64_t, uint32_t>(d_tmp, (size_t)T)));  // one scratch for the four passes
    // least significant word first; every later pass is stable, so the order of the earlier words holds among equals
    for (int w = 0; w < 4; w++) {
      hipLaunchKernelGGL(k_word, grdT, blk, 0, 0, (const u256*)d_keys.p, w == 0 ? (const uint32_t*)nullptr : (const uint32_t*)i_in,
                         T, w, w_in, i_in);
      G2S_HIP_TRY(radix_sort_pairs(d_tmp, w_in, w_out, i_in, i_out, (size_t)T));
      std::swap(i_in, i_out);
    }
    d_lo.free(); d_lo2.free(); d_tmp.free();
    G2S_HIP_TRY(d_alt.alloc((size_t)T * sizeof(KT)));
    hipLaunchKernelGGL(k_gather, grdT, blk, 0, 0, (const u256*)d_keys.p, (const uint32_t*)i_in, T, (u256*)d_alt.p);
    d_hi.free(); d_hi2.free(); d_keys.free();
    sorted = (KT*)d_alt.p;
  } else {
    G2S_HIP_TRY(d_lo.alloc((size_t)T * 8));
    G2S_HIP_TRY(d_hi.alloc((size_t)T * 8));
    G2S_HIP_TRY(d_lo2.alloc((size_t)T * 8));
    G2S_HIP_TRY(d_hi2.alloc((size_t)T * 8));
    hipLaunchKernelGGL(k_split<KT>, grdT, blk, 0, 0, (const KT*)d_keys.p, T, (uint64_t*)d_lo.p, (uint64_t*)d_hi.p);
    // least significant word first, then a stable pass on the most significant word (the first call's scratch serves both)
    G2S_HIP_TRY(radix_sort_pairs(d_tmp, (uint64_t*)d_lo.p, (uint64_t*)d_lo2.p, (uint64_t*)d_hi.p, (uint64_t*)d_hi2.p, (size_t)T));
    G2S_HIP_TRY(radix_sort_pairs(d_tmp, (uint64_t*)d_hi2.p, (uint64_t*)d_hi.p, (uint64_t*)d_lo2.p, (uint64_t*)d_lo.p, (size_t)T));
    hipLaunchKernelGGL(k_join, grdT, blk, 0, 0, (const uint64_t*)d_lo.p, (const uint64_t*)d_hi.p, T, (u128*)d_keys.p);
    sorted = (KT*)d_keys.p;
    d_lo2.free(); d_hi2.free();
  }
  // ---- runs of equal keys -> the k-mers seen at least `solid` times
  G2S_HIP_TRY(d_flag.alloc((size_t)T * 4));
  G2S_HIP_TRY(d_pos.alloc((size_t)T * 4));
  hipLaunchKernelGGL(k_heads<KT>, grdT, blk, 0, 0, (const KT*)sorted, T, (uint32_t*)d_flag.p);
  Scratch d_tmp2;
  uint32_t nheads = 0, n_solid = 0;
  G2S_HIP_TRY(scan_total(d_tmp2, (const uint32_t*)d_flag.p, (uint32_t*)d_pos.p, (size_t)T, &nheads));
  if (nheads) {
    G2S_HIP_TRY(d_hidx.alloc((size_t)nheads * 4));
    G2S_HIP_TRY(d_keep.alloc((size_t)nheads * 4));
    G2S_HIP_TRY(d_kpos.alloc((size_t)nheads * 4));
    G2S_HIP_TRY(hipMemset(d_misc.p, 0, 16));
    hipLaunchKernelGGL(k_head_index<KT>, grdT, blk, 0, 0, (const KT*)sorted, (const uint32_t*)d_flag.p,
                       (const uint32_t*)d_pos.p, T, (uint32_t*)d_hidx.p, (uint32_t*)d_misc.p);
    uint32_t n_valid = 0;
    G2S_HIP_TRY(hipMemcpy(&n_valid, d_misc.p, 4, hipMemcpyDeviceToHost));
    const dim3 grdH((nheads + 255) / 256);
    hipLaunchKernelGGL(k_solid_flag, grdH, blk, 0, 0, (const uint32_t*)d_hidx.p, nheads, n_valid, (uint32_t)std::max(1, solid),
                       (uint32_t*)d_keep.p);
    Scratch d_tmp3;
    G2S_HIP_TRY(scan_total(d_tmp3, (const uint32_t*)d_keep.p, (uint32_t*)d_kpos.p, (size_t)nheads, &n_solid));
    if (n_solid) {
      G2S_HIP_TRY(d_out.alloc((size_t)n_solid * sizeof(KT)));
      hipLaunchKernelGGL(k_compact<KT>, grdH, blk, 0, 0, (const KT*)sorted, (const uint32_t*)d_hidx.p,
                         (const uint32_t*)d_keep.p, (const uint32_t*)d_kpos.p, nheads, (KT*)d_out.p);
    }
  }
  G2S_HIP_TRY(hipGetLastError());
  // ---- with reach records: the kept part of the set takes the set's place (graph_reach.h)
  if (in.reach) {
    GraphReachInfo rinfo;
    uint64_t nkept = 0;
    DevMem d_kept;
    // (the sort's buffers are read for the last time by k_compact: the search's index, bitmap and queue take their room)
    G2S_HIP_TRY(hipDeviceSynchronize());
    d_keys.free(); d_alt.free(); d_lo.free(); d_hi.free(); d_lo2.free(); d_hi2.free(); d_flag.free(); d_pos.free();
    d_hidx.free(); d_keep.free(); d_kpos.free(); d_tmp.free(); d_tmp2.free();
    if (n_solid && !reach_on_device<KT>((const KT*)d_out.p, (uint64_t)n_solid, k, *in.reach, d_kept, &nkept, why, &rinfo)) return false;
    if (!n_solid) { rinfo.records = in.reach->records; rinfo.seeds = in.reach->seed.size(); rinfo.on_device = 1; }
    set_graph_reach_info(rinfo);
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s]   reach: %llu of %llu k-mers kept on the GPU, %u levels, the queue grown %u times\n",
              (unsigned long long)nkept, (unsigned long long)n_solid, rinfo.levels, rinfo.regrowths);
    if (nkept >= graph_max_kmers()) {  // (graph_build refuses it: nothing comes down)
      out.clear();
      g.n = nkept;
      g.bucket.clear();
      return true;
    }
    d_out.free();
    d_out = std::move(d_kept);
    n_solid = (uint32_t)nkept;
  }
  // ---- prefix index and the copies the host keeps (node look-ups, node strings)
  const int bits = std::min(2 * k, 22);
  const uint32_t nb = 1u << bits;
  std::vector<uint32_t> bucket((size_t)nb + 1, 0);
  std::vector<KT> host((size_t)n_solid);
  if (n_solid) {
    DevMem d_bucket;
    G2S_HIP_TRY(d_bucket.alloc(((size_t)nb + 1) * 4));
    hipLaunchKernelGGL(k_bucket<KT>, dim3((nb + 1 + 255) / 256), blk, 0, 0, (const KT*)d_out.p, n_solid, 2 * k - bits, nb,
                       (uint32_t*)d_bucket.p);
    G2S_HIP_TRY(hipMemcpy(bucket.data(), d_bucket.p, ((size_t)nb + 1) * 4, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(host.data(), d_out.p, (size_t)n_solid * sizeof(KT), hipMemcpyDeviceToHost));
  }
  out.swap(host);
  g.n = n_solid;
  g.bucket.swap(bucket);
  g.bucket_bits = bits;
  return true;
}

// T keys sorted by (set, k-mer), or by k-mer alone without set ids (d_sid / d_ss == nullptr): LSD passes over the
// k-mer's 64-bit words, then one stable pass over the set id, as (word, index) pairs with one gather at the end.
// d_keys and d_sid are consumed; the sorted copies land in d_sk / d_ss.
template <class KT>
static bool sort_keyed_gpu(DevMem& d_keys, DevMem* d_sid, uint64_t T, DevMem& d_sk, DevMem* d_ss, std::string* why) {
  DevMem d_w0, d_w1, d_i0, d_i1;
  Scratch d_tmp;
  const dim3 blk(256), grdT((unsigned)((T + 255) / 256));
  G2S_HIP_TRY(d_w0.alloc((size_t)T * 8));
  G2S_HIP_TRY(d_w1.alloc((size_t)T * 8));
  G2S_HIP_TRY(d_i0.alloc((size_t)T * 4));
  G2S_HIP_TRY(d_i1.alloc((size_t)T * 4));
  uint64_t *w_in = (uint64_t*)d_w0.p, *w_out = (uint64_t*)d_w1.p;
  uint32_t *i_in = (uint32_t*)d_i0.p, *i_out = (uint32_t*)d_i1.p;
  G2S_HIP_TRY((radix_sort_pairs_reserve<uint64_t, uint32_t>(d_tmp, (size_t)T)));  // one scratch for every pass
  constexpr int W = (int)(sizeof(KT) / 8);
  const uint32_t* sid = d_sid ? (const uint32_t*)d_sid->p : nullptr;
  for (int w = 0; w < (sid ? W + 1 : W); w++) {
    const int word = w < W ? w : -1;
    hipLaunchKernelGGL(k_key_word<KT>, grdT, blk, 0, 0, (const KT*)d_keys.p, sid,
                       w == 0 ? (const uint32_t*)nullptr : (const uint32_t*)i_in, T, word, w_in, i_in);
    G2S_HIP_TRY(radix_sort_pairs(d_tmp, w_in, w_out, i_in, i_out, (size_t)T, word < 0 ? 32 : 64));
    std::swap(i_in, i_out);
  }
  d_w0.free(); d_w1.free(); d_tmp.free();
  G2S_HIP_TRY(d_sk.alloc((size_t)T * sizeof(KT)));
  if (sid) {
    G2S_HIP_TRY(d_ss->alloc((size_t)T * 4));
    hipLaunchKernelGGL(k_gather_keyed<KT>, grdT, blk, 0, 0, (const KT*)d_keys.p, sid, (const uint32_t*)i_in, T, (KT*)d_sk.p,
                       (uint32_t*)d_ss->p);
    d_sid->free();
  } else {
    hipLaunchKernelGGL(k_gather_keys<KT>, grdT, blk, 0, 0, (const KT*)d_keys.p, (const uint32_t*)i_in, T, (KT*)d_sk.p);
  }
  G2S_HIP_TRY(hipGetLastError());
  d_keys.free();
  return true;
}

// the runs of equal (set, k-mer) in T sorted keys: run j = [hidx[j], tidx[j]]
template <class KT>
static bool runs_keyed_gpu(const KT* sk, const uint32_t* ss, uint64_t T, DevMem& d_hidx, DevMem& d_tidx, uint32_t* nruns_out, std::string* why) {
  DevMem d_flag, d_pos;
  Scratch d_tmp2;
  const dim3 blk(256), grdT((unsigned)((T + 255) / 256));
  G2S_HIP_TRY(d_flag.alloc((size_t)T * 4));
  G2S_HIP_TRY(d_pos.alloc((size_t)T * 4));
  hipLaunchKernelGGL(k_heads_keyed<KT>, grdT, blk, 0, 0, sk, ss, T, (uint32_t*)d_flag.p);
  uint32_t nruns = 0;
  G2S_HIP_TRY(scan_total(d_tmp2, (const uint32_t*)d_flag.p, (uint32_t*)d_pos.p, (size_t)T, &nruns));
  if (nruns) {
    G2S_HIP_TRY(d_hidx.alloc((size_t)nruns * 4));
    G2S_HIP_TRY(d_tidx.alloc((size_t)nruns * 4));
    hipLaunchKernelGGL(k_runs_keyed<KT>, grdT, blk, 0, 0, sk, ss, (const uint32_t*)d_flag.p, (const uint32_t*)d_pos.p, T,
                       (uint32_t*)d_hidx.p, (uint32_t*)d_tidx.p);
  }
  *nruns_out = nruns;
  return true;
}

// The solid k-mer sets of a set graph at once: one key per text position (all sets' sequences in one text, the set
// from a per-sequence table), sorted by (set, canonical k-mer) — LSD passes over the k-mer's 64-bit words, then one
// stable pass over the set id, as (word, index) pairs with one gather at the end — runs over (set, k-mer), solidity per
// run, compaction, every set's first rank.  out / rank_set / g.set_lo set-major; false (g untouched) when the device
// cannot be used.
template <class KT>
static bool count_solid_sets_gpu_t(Graph& g, std::vector<uint32_t>* rank_set, const std::vector<std::pair<const char*, uint64_t>>& seqs,
                                   const std::vector<uint32_t>& seq_set, uint32_t nsets, int solid, int device, std::string* why) {
  std::vector<KT>& out = kmer_vec<KT>(g);
  if (!device_exists(device)) { if (why) *why = "no device"; return false; }
  G2S_HIP_TRY(hipSetDevice(device));
  const int k = g.k;
  uint64_t T = 0;
  for (auto& sq : seqs) T += sq.second + 1;  // one separator after every sequence
  if (T == 0 || T >= (1ull << 32) || seqs.empty()) { if (why) *why = "text size"; return false; }
  size_t free_b = 0, total_b = 0;
  G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  // (bytes a text position at the peak: keys, set ids, word and index double buffers, the sort's scratch, the gathered copies)
  const double per_pos = (double)(2 * sizeof(KT) + 56);
  if ((double)T * per_pos > 0.5 * (double)free_b) { if (why) *why = "text too large for the device"; return false; }
  std::vector<uint8_t> text((size_t)T);
  std::vector<uint64_t> start(seqs.size());
  {
    size_t pos = 0;
    for (size_t j = 0; j < seqs.size(); j++) {
      start[j] = pos;
      memcpy(text.data() + pos, seqs[j].first, (size_t)seqs[j].second);
      pos += (size_t)seqs[j].second;
      text[pos++] = 'N';
    }
  }
  const uint32_t ns = (uint32_t)seqs.size();
  DevMem d_text, d_start, d_sset, d_keys, d_sid, d_sk, d_ss, d_hidx, d_tidx, d_keep, d_kpos, d_out, d_osid, d_lo;
  G2S_HIP_TRY(d_text.alloc((size_t)T));
  G2S_HIP_TRY(d_start.alloc((size_t)ns * 8));
  G2S_HIP_TRY(d_sset.alloc((size_t)ns * 4));
  G2S_HIP_TRY(d_keys.alloc((size_t)T * sizeof(KT)));
  G2S_HIP_TRY(d_sid.alloc((size_t)T * 4));
  G2S_HIP_TRY(hipMemcpy(d_text.p, text.data(), (size_t)T, hipMemcpyHostToDevice));
  G2S_HIP_TRY(hipMemcpy(d_start.p, start.data(), (size_t)ns * 8, hipMemcpyHostToDevice));
  G2S_HIP_TRY(hipMemcpy(d_sset.p, seq_set.data(), (size_t)ns * 4, hipMemcpyHostToDevice));
  const dim3 blk(256), grdT((unsigned)((T + 255) / 256));
  hipLaunchKernelGGL(k_extract<KT>, grdT, blk, 0, 0, (const uint8_t*)d_text.p, T, k, (KT*)d_keys.p);
  hipLaunchKernelGGL(k_pos_set, grdT, blk, 0, 0, (const uint64_t*)d_start.p, (const uint32_t*)d_sset.p, ns, T, (uint32_t*)d_sid.p);
  d_text.free(); d_start.free(); d_sset.free();
  // ---- sort by (set, k-mer), then the runs -> the k-mers seen at least `solid` times in their own set
  if (!sort_keyed_gpu<KT>(d_keys, &d_sid, T, d_sk, &d_ss, why)) return false;
  const KT* sk = (const KT*)d_sk.p;
  const uint32_t* ss = (const uint32_t*)d_ss.p;
  uint32_t nruns = 0;
  if (!runs_keyed_gpu<KT>(sk, ss, T, d_hidx, d_tidx, &nruns, why)) return false;
  uint32_t n_solid = 0;
  if (nruns) {
    G2S_HIP_TRY(d_keep.alloc((size_t)nruns * 4));
    G2S_HIP_TRY(d_kpos.alloc((size_t)nruns * 4));
    const dim3 grdR((nruns + 255) / 256);
    hipLaunchKernelGGL(k_solid_keyed, grdR, blk, 0, 0, (const uint32_t*)d_hidx.p, (const uint32_t*)d_tidx.p, nruns,
                       (uint32_t)std::max(1, solid), (uint32_t*)d_keep.p);
    Scratch d_tmp3;
    G2S_HIP_TRY(scan_total(d_tmp3, (const uint32_t*)d_keep.p, (uint32_t*)d_kpos.p, (size_t)nruns, &n_solid));
    if (n_solid) {
      G2S_HIP_TRY(d_out.alloc((size_t)n_solid * sizeof(KT)));
      G2S_HIP_TRY(d_osid.alloc((size_t)n_solid * 4));
      hipLaunchKernelGGL(k_compact_keyed<KT>, grdR, blk, 0, 0, sk, ss, (const uint32_t*)d_hidx.p, (const uint32_t*)d_keep.p,
                         (const uint32_t*)d_kpos.p, nruns, (KT*)d_out.p, (uint32_t*)d_osid.p);
    }
  }
  // ---- every set's first rank
  std::vector<uint32_t> lo32((size_t)nsets + 1, 0);
  std::vector<KT> host((size_t)n_solid);
  std::vector<uint32_t> rs((size_t)n_solid);
  if (n_solid) {
    G2S_HIP_TRY(d_lo.alloc(((size_t)nsets + 1) * 4));
    hipLaunchKernelGGL(k_set_first, dim3((nsets + 1 + 255) / 256), blk, 0, 0, (const uint32_t*)d_osid.p, n_solid, nsets, (uint32_t*)d_lo.p);
    G2S_HIP_TRY(hipMemcpy(lo32.data(), d_lo.p, lo32.size() * 4, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(host.data(), d_out.p, (size_t)n_solid * sizeof(KT), hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(rs.data(), d_osid.p, (size_t)n_solid * 4, hipMemcpyDeviceToHost));
  }
  G2S_HIP_TRY(hipGetLastError());
  out.swap(host);
  rank_set->swap(rs);
  g.n = n_solid;
  g.set_lo.assign(lo32.begin(), lo32.end());
  return true;
}

bool graph_build_sets_gpu(Graph& g, const std::vector<std::pair<const char*, uint64_t>>& seqs, const std::vector<uint32_t>& seq_set,
                          uint32_t nsets, int solid, int device,
                          const std::function<void(const std::vector<uint32_t>&, uint32_t)>& host_walk, std::string* why) {
  return with_kmer_type(g.kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    std::vector<uint32_t> rank_set;
    return count_solid_sets_gpu_t<KT>(g, &rank_set, seqs, seq_set, nsets, solid, device, why) &&
           finish_gpu_t<KT>(g, device, host_walk, why, &rank_set);
  });
}

// The solid k-mer sets of a pooled set graph (dbg.hpp: PoolSets).  The expanded lists are never formed: the text of the
// pool's sequences that some list names goes up once and gives one key per pool position; the own lists' (key, set)
// pairs and the shared list's keys are gathered from those; the own pairs take the keyed sort and run detection of
// count_solid_sets_gpu_t; the shared keys are sorted ONCE and run-length counted, however many sets hold them; the two
// tables are merged per set into the (set, k-mer) order the rest of the build wants.  info: positions and keys sorted.
template <class KT>
static bool count_solid_pool_gpu_t(Graph& g, std::vector<uint32_t>* rank_set, const PoolSets& ps, int solid, int device,
                                   PoolBuildInfo* info, std::string* why, const PoolReach* reach, PoolReachInfo* rinfo,
                                   bool* device_usable) {
  std::vector<KT>& out = kmer_vec<KT>(g);
  if (!device_exists(device)) { if (why) *why = "no device"; return false; }
  G2S_HIP_TRY(hipSetDevice(device));
  if (device_usable) *device_usable = true;  // (a failure from here on is the device build giving up, not its absence)
  const int k = g.k;
  const std::vector<std::pair<const char*, uint64_t>>& seqs = *ps.seqs;
  const uint32_t nsets = ps.nsets;
  // ---- the instances, and the pool sequences they name (numbered in order of first use)
  std::vector<uint32_t> local(seqs.size(), INV), used;
  auto use = [&](uint32_t j) -> uint32_t {
    if (local[j] == INV) { local[j] = (uint32_t)used.size(); used.push_back(j); }
    return local[j];
  };
  const uint64_t q0 = ps.set_begin[0], ninst64 = ps.set_begin[nsets] - q0;
  if (ninst64 >= (1ull << 32) || ps.nshared >= (1ull << 32)) { if (why) *why = "text size"; return false; }
  std::vector<uint32_t> inst_seq((size_t)ninst64), inst_set((size_t)ninst64), set_fidx(nsets, INV), fset, sh_seq;
  uint64_t I = 0, S = 0, P = 0;  // positions (bases + 1) of the own instances, of the shared list, of the pool in use
  for (uint32_t s = 0; s < nsets; s++) {
    for (uint64_t q = ps.set_begin[s]; q < ps.set_begin[s + 1]; q++) {
      inst_seq[(size_t)(q - q0)] = use(ps.set_seq[q]);
      inst_set[(size_t)(q - q0)] = s;
      I += seqs[ps.set_seq[q]].second + 1;
    }
    if (ps.flagged(s)) { set_fidx[s] = (uint32_t)fset.size(); fset.push_back(s); }
  }
  uint32_t F = (uint32_t)fset.size();
  if (F)
    for (uint64_t x = 0; x < ps.nshared; x++) {
      sh_seq.push_back(use(ps.shared_seq[x]));
      S += seqs[ps.shared_seq[x]].second + 1;
    }
  const uint32_t nu = (uint32_t)used.size(), ninst = (uint32_t)ninst64, nsh = (uint32_t)sh_seq.size();
  // the text: the sequences with a host pointer in order of first use, packed here and uploaded; behind them those
  // that lie in a device-held pool (a null pointer: PoolSets::device_text), gathered where they are
  std::vector<uint32_t> seq_start(nu), seq_len1(nu);
  auto in_pool = [&](uint32_t j) { return ps.device_text != nullptr && seqs[j].first == nullptr; };
  uint64_t PH = 0;  // the positions of the host part
  for (int part = 0; part < 2; part++) {
    for (uint32_t u = 0; u < nu && P < (1ull << 32); u++) {
      if (in_pool(used[u]) != (part == 1)) continue;
      const uint64_t len = std::min<uint64_t>(seqs[used[u]].second, 1ull << 32);  // (a longer one fails the guard below)
      seq_start[u] = (uint32_t)P;
      seq_len1[u] = (uint32_t)(len + 1);
      P += len + 1;
    }
    if (part == 0) PH = P;
  }
  // (instance positions + shared positions below 2^32, as the set build wants of its text; the pool in use is no larger)
  if (I + S == 0 || I + S >= (1ull << 32) || P >= (1ull << 32)) { if (why) *why = "text size"; return false; }
  size_t free_b = 0, total_b = 0;
  G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  // (the pool's text and keys while the pairs are gathered; a gathered position at its sort's peak as in
  // count_solid_sets_gpu_t; the merge is checked once the shared table's size is known)
  if ((double)P * (double)(sizeof(KT) + 1) + (double)(I + S) * (double)(2 * sizeof(KT) + 56) > 0.5 * (double)free_b) {
    if (why) *why = "text too large for the device";
    return false;
  }
  std::vector<uint8_t> text((size_t)PH);
  // (what k_gather_reads is told of every read it copies, as four arrays of ng entries in one: pool, read in the pool,
  // place in the text, length + 1)
  std::vector<GatherSource> g_table;
  size_t ng = 0;
  for (uint32_t u = 0; u < nu; u++) ng += in_pool(used[u]) ? 1 : 0;
  std::vector<uint32_t> g_rows(4 * ng);
  size_t gi = 0;
  if (P > PH)
    for (const PoolDeviceText& d : *ps.device_text) g_table.push_back(GatherSource{d.text, d.start});
  for (uint32_t u = 0; u < nu; u++) {
    const uint32_t j = used[u];
    if (!in_pool(j)) {
      memcpy(text.data() + seq_start[u], seqs[j].first, (size_t)seqs[j].second);
      text[(size_t)seq_start[u] + seq_len1[u] - 1] = 'N';  // one separator after every sequence
      continue;
    }
    // the pool that holds j: the last one that begins at or before it
    const std::vector<PoolDeviceText>& dv = *ps.device_text;
    size_t lo = 0, hi = dv.size();
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) / 2;
      if (dv[mid].first <= j) lo = mid; else hi = mid;
    }
    if (dv.empty() || j < dv[lo].first || (uint64_t)(j - dv[lo].first) >= dv[lo].n_reads || dv[lo].device != device) {
      if (why) *why = "a sequence in no pool of this device";
      return false;
    }
    g_rows[gi] = (uint32_t)lo;
    g_rows[ng + gi] = j - dv[lo].first;
    g_rows[2 * ng + gi] = seq_start[u];
    g_rows[3 * ng + gi] = seq_len1[u];
    gi++;
  }
  const dim3 blk(256);
  auto grid = [](uint64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  DevMem d_keys, d_sid, d_hkeys;
  {
    DevMem d_text, d_pkeys, d_sstart, d_slen1, d_iseq, d_iset, d_ilen, d_istart;
    G2S_HIP_TRY(d_text.alloc((size_t)P));
    G2S_HIP_TRY(d_pkeys.alloc((size_t)P * sizeof(KT)));
    G2S_HIP_TRY(d_sstart.alloc((size_t)nu * 4));
    G2S_HIP_TRY(d_slen1.alloc((size_t)nu * 4));
    if (PH) G2S_HIP_TRY(hipMemcpy(d_text.p, text.data(), (size_t)PH, hipMemcpyHostToDevice));
    if (ng) {
      // (one allocation: the pools' table, then the four arrays — an allocation costs more than the kernel)
      const size_t tab_bytes = (g_table.size() * sizeof(GatherSource) + 255) & ~(size_t)255;
      DevMem d_g;
      G2S_HIP_TRY(d_g.alloc(tab_bytes + 4 * ng * 4));
      const uint32_t* rows = (const uint32_t*)(d_g.as<uint8_t>() + tab_bytes);
      G2S_HIP_TRY(hipMemcpy(d_g.p, g_table.data(), g_table.size() * sizeof(GatherSource), hipMemcpyHostToDevice));
      G2S_HIP_TRY(hipMemcpy(d_g.as<uint8_t>() + tab_bytes, g_rows.data(), 4 * ng * 4, hipMemcpyHostToDevice));
      const unsigned ggroups = (unsigned)std::min<uint64_t>(((uint64_t)ng + 3) / 4, 256u * 16u);
      hipLaunchKernelGGL(k_gather_reads, dim3(ggroups), blk, 0, 0, (const GatherSource*)d_g.p, rows, rows + ng, rows + 2 * ng,
                         rows + 3 * ng, (uint32_t)ng, (uint8_t*)d_text.p, P);
      G2S_HIP_TRY(hipGetLastError());
      G2S_HIP_TRY(hipDeviceSynchronize());  // (the tables go with this scope)
    }
    G2S_HIP_TRY(hipMemcpy(d_sstart.p, seq_start.data(), (size_t)nu * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_slen1.p, seq_len1.data(), (size_t)nu * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_extract<KT>, grid(P), blk, 0, 0, (const uint8_t*)d_text.p, P, k, (KT*)d_pkeys.p);
    // the own lists' pairs, then the shared list's keys: instance -> pool position through the instances' start table
    for (int pass = 0; pass < 2; pass++) {
      const uint32_t ni = pass == 0 ? ninst : nsh;
      const uint64_t np = pass == 0 ? I : S;
      if (!np) continue;
      G2S_HIP_TRY(d_iseq.alloc((size_t)ni * 4));
      G2S_HIP_TRY(d_ilen.alloc((size_t)ni * 4));
      G2S_HIP_TRY(d_istart.alloc((size_t)ni * 4));
      G2S_HIP_TRY(hipMemcpy(d_iseq.p, pass == 0 ? inst_seq.data() : sh_seq.data(), (size_t)ni * 4, hipMemcpyHostToDevice));
      if (pass == 0) {
        G2S_HIP_TRY(d_iset.alloc((size_t)ni * 4));
        G2S_HIP_TRY(hipMemcpy(d_iset.p, inst_set.data(), (size_t)ni * 4, hipMemcpyHostToDevice));
        G2S_HIP_TRY(d_sid.alloc((size_t)np * 4));
      }
      DevMem& d_dst = pass == 0 ? d_keys : d_hkeys;
      G2S_HIP_TRY(d_dst.alloc((size_t)np * sizeof(KT)));
      hipLaunchKernelGGL(k_inst_len, grid(ni), blk, 0, 0, (const uint32_t*)d_iseq.p, (const uint32_t*)d_slen1.p, ni, (uint32_t*)d_ilen.p);
      G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_ilen.p, (uint32_t*)d_istart.p, (size_t)ni));
      hipLaunchKernelGGL(k_pool_pairs<KT>, grid(np), blk, 0, 0, (const KT*)d_pkeys.p, (const uint32_t*)d_istart.p,
                         (const uint32_t*)d_iseq.p, pass == 0 ? (const uint32_t*)d_iset.p : (const uint32_t*)nullptr,
                         (const uint32_t*)d_sstart.p, ni, np, (KT*)d_dst.p, pass == 0 ? (uint32_t*)d_sid.p : (uint32_t*)nullptr);
      G2S_HIP_TRY(hipGetLastError());
      d_iseq.free(); d_iset.free(); d_ilen.free(); d_istart.free();
    }
  }
  info->own_positions = I;
  info->shared_positions = S;
  info->keys_sorted = 0;
  info->text_gathered = P - PH;
  info->text_packed = PH;
  // ---- the own lists: (set, k-mer) sort, runs, the run table and every set's first run
  DevMem d_rkey, d_rset, d_rcnt, d_rlo;
  uint32_t nruns = 0;
  if (I) {
    DevMem d_sk, d_ss, d_hidx, d_tidx;
    if (!sort_keyed_gpu<KT>(d_keys, &d_sid, I, d_sk, &d_ss, why)) return false;
    info->keys_sorted += I;
    if (!runs_keyed_gpu<KT>((const KT*)d_sk.p, (const uint32_t*)d_ss.p, I, d_hidx, d_tidx, &nruns, why)) return false;
    G2S_HIP_TRY(d_rkey.alloc((size_t)nruns * sizeof(KT)));
    G2S_HIP_TRY(d_rset.alloc((size_t)nruns * 4));
    G2S_HIP_TRY(d_rcnt.alloc((size_t)nruns * 4));
    if (nruns) {
      hipLaunchKernelGGL(k_run_table<KT>, grid(nruns), blk, 0, 0, (const KT*)d_sk.p, (const uint32_t*)d_ss.p, (const uint32_t*)d_hidx.p,
                         (const uint32_t*)d_tidx.p, nruns, (KT*)d_rkey.p, (uint32_t*)d_rset.p, (uint32_t*)d_rcnt.p);
    }
    G2S_HIP_TRY(hipDeviceSynchronize());
  } else {
    G2S_HIP_TRY(d_rkey.alloc(0));
    G2S_HIP_TRY(d_rset.alloc(0));
    G2S_HIP_TRY(d_rcnt.alloc(0));
  }
  G2S_HIP_TRY(d_rlo.alloc(((size_t)nsets + 1) * 4));
  hipLaunchKernelGGL(k_set_first, grid((uint64_t)nsets + 1), blk, 0, 0, (const uint32_t*)d_rset.p, nruns, nsets, (uint32_t*)d_rlo.p);
  // ---- the shared list: sorted once as plain k-mers, run-length counted
  DevMem d_hkey, d_hcnt;
  uint32_t U = 0;
  if (S) {
    DevMem d_hs, d_flag, d_pos, d_hidx, d_misc;
    if (!sort_keyed_gpu<KT>(d_hkeys, nullptr, S, d_hs, nullptr, why)) return false;
    info->keys_sorted += S;
    G2S_HIP_TRY(d_flag.alloc((size_t)S * 4));
    G2S_HIP_TRY(d_pos.alloc((size_t)S * 4));
    G2S_HIP_TRY(d_misc.alloc(16));
    hipLaunchKernelGGL(k_heads<KT>, grid(S), blk, 0, 0, (const KT*)d_hs.p, S, (uint32_t*)d_flag.p);
    // (not scan_total: the scan's scratch is freed before the two copies, as the pool build always did)
    G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_flag.p, (uint32_t*)d_pos.p, (size_t)S));
    G2S_HIP_TRY(read_total((const uint32_t*)d_flag.p, (const uint32_t*)d_pos.p, (size_t)S, &U));
    if (U) {
      G2S_HIP_TRY(d_hidx.alloc((size_t)U * 4));
      G2S_HIP_TRY(d_hkey.alloc((size_t)U * sizeof(KT)));
      G2S_HIP_TRY(d_hcnt.alloc((size_t)U * 4));
      G2S_HIP_TRY(hipMemset(d_misc.p, 0, 16));
      hipLaunchKernelGGL(k_head_index<KT>, grid(S), blk, 0, 0, (const KT*)d_hs.p, (const uint32_t*)d_flag.p, (const uint32_t*)d_pos.p, S,
                         (uint32_t*)d_hidx.p, (uint32_t*)d_misc.p);
      uint32_t n_valid = 0;
      G2S_HIP_TRY(hipMemcpy(&n_valid, d_misc.p, 4, hipMemcpyDeviceToHost));
      hipLaunchKernelGGL(k_shared_table<KT>, grid(U), blk, 0, 0, (const KT*)d_hs.p, (const uint32_t*)d_hidx.p, U, n_valid,
                         (KT*)d_hkey.p, (uint32_t*)d_hcnt.p);
      G2S_HIP_TRY(hipDeviceSynchronize());
    }
  }
  if (!U) {
    G2S_HIP_TRY(d_hkey.alloc(0));
    G2S_HIP_TRY(d_hcnt.alloc(0));
  }
  // ---- the sets with a reach record (dbg.hpp: PoolReach): a bounded search per set over the two tables; what it kept
  // replaces those sets' runs (as runs of `solid` copies) and the sets lose their flag, so that the merge below keeps
  // exactly the kept k-mers for them and its flagged sets x shared k-mers items are those of the sets without a record
  if (reach && reach->any()) {
    const uint32_t so = (uint32_t)std::max(1, solid);
    std::vector<uint32_t> rsets, set_ridx(nsets, INV), set_fr(nsets, INV), seed_lo(1, 0), run_lo((size_t)nsets + 1);
    std::vector<int32_t> radius;
    std::vector<KT> seeds;
    uint32_t rows = 0;
    G2S_HIP_TRY(hipMemcpy(run_lo.data(), d_rlo.p, run_lo.size() * 4, hipMemcpyDeviceToHost));
    uint64_t upper = 0, own_rec = 0;  // the k-mers the searches can visit at most; the own runs among them
    for (uint32_t s = 0; s < nsets; s++) {
      if (!reach->has(s)) continue;
      set_ridx[s] = (uint32_t)rsets.size();
      rsets.push_back(s);
      radius.push_back(reach->radius[s]);
      if (set_fidx[s] != INV && U) set_fr[s] = rows++;
      own_rec += (uint64_t)(run_lo[s + 1] - run_lo[s]);
      upper += (uint64_t)(run_lo[s + 1] - run_lo[s]) + (set_fr[s] != INV ? U : 0u);
      for (uint64_t q = reach->seed_begin[s]; q < reach->seed_begin[s + 1]; q++) {
        KT c;
        int strand;
        encode_kmer<KT>(reach->seed[(size_t)q], k, &c, &strand);
        seeds.push_back(c);
      }
      if (seeds.size() >= (1ull << 32)) { if (why) *why = "reach: 2^32 seeds or more"; return false; }
      seed_lo.push_back((uint32_t)seeds.size());
    }
    const uint32_t R = (uint32_t)rsets.size(), W = (U + 31u) / 32u;
    const size_t own_words = ((size_t)nruns + 31) / 32, sh_words = (size_t)rows * W;
    G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // (a queued k-mer: the queue, then the sort of count_solid_sets_gpu_t over what was queued; the bitmaps beside it)
    const double per_item = (double)(2 * sizeof(KT) + 56), bitmap_bytes = (double)(own_words + sh_words) * 4.0;
    if (bitmap_bytes > 0.25 * (double)free_b) { if (why) *why = "reach: visited bitmaps too large for the device"; return false; }
    // The queue is sized by what the searches can plausibly keep, not by sets x shared k-mers: the own runs of the sets
    // with a record plus kReachShare k-mers a set; when it overflows it is made four times as large and the searches
    // run again (bitmaps cleared), up to `cap`: what the sets could hold at most, what fits half the free memory, 2^31 - 1.
    // (G2S_REACH_QUEUE_CAP: the tests make the queue small, and final, to take the overflow path)
    constexpr uint64_t kReachShare = 4096;
    uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(upper, 1), (1ull << 31) - 1);
    cap = std::min<uint64_t>(cap, (uint64_t)std::max(1.0, (0.5 * (double)free_b - bitmap_bytes) / per_item));
    if (getenv("G2S_REACH_QUEUE_CAP")) cap = std::min<uint64_t>(cap, (uint64_t)std::max(1ll, atoll(getenv("G2S_REACH_QUEUE_CAP"))));
    uint64_t Q = std::min<uint64_t>(cap, own_rec + kReachShare * (uint64_t)rsets.size());
    const size_t own_bytes = std::max<size_t>(own_words * 4, 16), sh_bytes = std::max<size_t>(sh_words * 4, 16);
    DevMem d_rsets, d_radius, d_seedlo, d_setfr, d_ridx, d_seeds, d_ownb, d_shb, d_qkey, d_qset, d_ctl;
    G2S_HIP_TRY(d_rsets.alloc((size_t)R * 4));
    G2S_HIP_TRY(d_radius.alloc((size_t)R * 4));
    G2S_HIP_TRY(d_seedlo.alloc(((size_t)R + 1) * 4));
    G2S_HIP_TRY(d_setfr.alloc((size_t)nsets * 4));
    G2S_HIP_TRY(d_ridx.alloc((size_t)nsets * 4));
    G2S_HIP_TRY(d_seeds.alloc(seeds.size() * sizeof(KT)));
    G2S_HIP_TRY(d_ownb.alloc(own_bytes));
    G2S_HIP_TRY(d_shb.alloc(sh_bytes));
    G2S_HIP_TRY(d_ctl.alloc(16));
    G2S_HIP_TRY(hipMemcpy(d_rsets.p, rsets.data(), (size_t)R * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_radius.p, radius.data(), (size_t)R * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_seedlo.p, seed_lo.data(), ((size_t)R + 1) * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_setfr.p, set_fr.data(), (size_t)nsets * 4, hipMemcpyHostToDevice));
    G2S_HIP_TRY(hipMemcpy(d_ridx.p, set_ridx.data(), (size_t)nsets * 4, hipMemcpyHostToDevice));
    if (!seeds.empty()) G2S_HIP_TRY(hipMemcpy(d_seeds.p, seeds.data(), seeds.size() * sizeof(KT), hipMemcpyHostToDevice));
    ReachArgs ra;
    ra.rsets = (const uint32_t*)d_rsets.p;
    ra.radius = (const int32_t*)d_radius.p;
    ra.seed_lo = (const uint32_t*)d_seedlo.p;
    ra.set_fr = (const uint32_t*)d_setfr.p;
    ra.run_lo = (const uint32_t*)d_rlo.p;
    ra.rcnt = (const uint32_t*)d_rcnt.p;
    ra.hcnt = (const uint32_t*)d_hcnt.p;
    ra.own_bits = (uint32_t*)d_ownb.p;
    ra.sh_bits = (uint32_t*)d_shb.p;
    ra.ctl = (uint32_t*)d_ctl.p;
    ra.U = U; ra.W = W; ra.R = R; ra.solid = so; ra.k = k;
    uint32_t ctl[4] = {0, 0, 0, 0};
    for (;;) {
      G2S_HIP_TRY(d_qkey.alloc((size_t)Q * sizeof(KT)));
      G2S_HIP_TRY(d_qset.alloc((size_t)Q * 4));
      G2S_HIP_TRY(hipMemset(d_ownb.p, 0, own_bytes));
      G2S_HIP_TRY(hipMemset(d_shb.p, 0, sh_bytes));
      G2S_HIP_TRY(hipMemset(d_ctl.p, 0, 16));
      ra.out_set = (uint32_t*)d_qset.p;
      ra.Q = (uint32_t)Q;
      hipLaunchKernelGGL(k_reach_bfs<KT>, dim3(std::min<uint32_t>(R, 1024u)), dim3(kReachThreads), 0, 0, ra, (const KT*)d_rkey.p,
                         (const KT*)d_hkey.p, (const KT*)d_seeds.p, (KT*)d_qkey.p);
      G2S_HIP_TRY(hipGetLastError());
      G2S_HIP_TRY(hipMemcpy(ctl, d_ctl.p, 16, hipMemcpyDeviceToHost));
      if (!ctl[kReachOverflow]) break;
      if ((ctl[kReachOverflow] & kReachChunkListFull) || Q >= cap) {
        if (why) *why = "reach: the search's queue of " + std::to_string(Q) + " k-mers (or a level's chunk list) overflowed";
        return false;
      }
      if (getenv("G2S_DEBUG"))
        fprintf(stderr, "[g2s]   reach: the queue of %llu k-mers overflowed, searching again with %llu\n", (unsigned long long)Q,
                (unsigned long long)std::min<uint64_t>(cap, Q * 4));
      Q = std::min<uint64_t>(cap, Q * 4);
      d_qkey.free();
      d_qset.free();
    }
    const uint32_t nvis = ctl[kReachFill];
    d_ownb.free(); d_shb.free(); d_seeds.free();
    // the kept k-mers by (set, k-mer), every set's first; then the new run table
    DevMem d_sk, d_ss, d_vlo, d_ncnt, d_nlo, d_nkey, d_nset, d_nrc;
    G2S_HIP_TRY(d_vlo.alloc(((size_t)nsets + 1) * 4));
    if (nvis) {
      if (!sort_keyed_gpu<KT>(d_qkey, &d_qset, nvis, d_sk, &d_ss, why)) return false;
      hipLaunchKernelGGL(k_set_first, grid((uint64_t)nsets + 1), blk, 0, 0, (const uint32_t*)d_ss.p, nvis, nsets, (uint32_t*)d_vlo.p);
    } else {
      G2S_HIP_TRY(hipMemset(d_vlo.p, 0, ((size_t)nsets + 1) * 4));
      G2S_HIP_TRY(d_sk.alloc(0));
      G2S_HIP_TRY(d_ss.alloc(0));
    }
    G2S_HIP_TRY(d_ncnt.alloc(((size_t)nsets + 1) * 4));
    G2S_HIP_TRY(d_nlo.alloc(((size_t)nsets + 1) * 4));
    hipLaunchKernelGGL(k_reach_set_count, grid((uint64_t)nsets + 1), blk, 0, 0, (const uint32_t*)d_rlo.p, (const uint32_t*)d_ridx.p,
                       (const uint32_t*)d_vlo.p, nsets, (uint32_t*)d_ncnt.p);
    G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_ncnt.p, (uint32_t*)d_nlo.p, (size_t)nsets + 1));
    uint32_t nruns2 = 0;
    G2S_HIP_TRY(hipMemcpy(&nruns2, (const uint32_t*)d_nlo.p + nsets, 4, hipMemcpyDeviceToHost));
    G2S_HIP_TRY(d_nkey.alloc((size_t)nruns2 * sizeof(KT)));
    G2S_HIP_TRY(d_nset.alloc((size_t)nruns2 * 4));
    G2S_HIP_TRY(d_nrc.alloc((size_t)nruns2 * 4));
    if (nruns)
      hipLaunchKernelGGL(k_reach_copy_runs<KT>, grid(nruns), blk, 0, 0, (const KT*)d_rkey.p, (const uint32_t*)d_rset.p,
                         (const uint32_t*)d_rcnt.p, nruns, (const uint32_t*)d_ridx.p, (const uint32_t*)d_rlo.p, (const uint32_t*)d_nlo.p,
                         (KT*)d_nkey.p, (uint32_t*)d_nset.p, (uint32_t*)d_nrc.p);
    if (nvis)
      hipLaunchKernelGGL(k_reach_copy_kept<KT>, grid(nvis), blk, 0, 0, (const KT*)d_sk.p, (const uint32_t*)d_ss.p, nvis,
                         (const uint32_t*)d_vlo.p, (const uint32_t*)d_nlo.p, so, (KT*)d_nkey.p, (uint32_t*)d_nset.p, (uint32_t*)d_nrc.p);
    G2S_HIP_TRY(hipDeviceSynchronize());
    std::swap(d_rkey.p, d_nkey.p);
    std::swap(d_rset.p, d_nset.p);
    std::swap(d_rcnt.p, d_nrc.p);
    std::swap(d_rlo.p, d_nlo.p);
    nruns = nruns2;
    fset.clear();
    for (uint32_t s = 0; s < nsets; s++) {
      if (reach->has(s)) set_fidx[s] = INV;
      else if (set_fidx[s] != INV) { set_fidx[s] = (uint32_t)fset.size(); fset.push_back(s); }
    }
    F = (uint32_t)fset.size();
    rinfo->reach_sets = R;
    rinfo->kept_kmers = nvis;
    rinfo->full_kmers = 0;
    rinfo->full_known = 0;
    rinfo->levels = ctl[kReachLevels];
    rinfo->on_device = 1;
  }
  // ---- the merge: flags, scans, every set's count and first rank, then the writes — every buffer sized by its count
  const uint64_t FU64 = (uint64_t)F * U;
  if (FU64 + nruns >= (1ull << 31)) { if (why) *why = "size"; return false; }
  const uint32_t FU = (uint32_t)FU64, so = (uint32_t)std::max(1, solid);
  G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  // (two words an item for the flags and their scans, then at most one k-mer and its set id an item in the output)
  if ((double)(FU64 + nruns) * (double)(sizeof(KT) + 12) > 0.5 * (double)free_b) {
    if (why) *why = "merge too large for the device";
    return false;
  }
  DevMem d_sf, d_fset, d_kown, d_ksh, d_pown, d_psh, d_cnt, d_base, d_out, d_osid;
  G2S_HIP_TRY(d_sf.alloc((size_t)nsets * 4));
  G2S_HIP_TRY(d_fset.alloc((size_t)F * 4));
  G2S_HIP_TRY(hipMemcpy(d_sf.p, set_fidx.data(), (size_t)nsets * 4, hipMemcpyHostToDevice));
  if (F) G2S_HIP_TRY(hipMemcpy(d_fset.p, fset.data(), (size_t)F * 4, hipMemcpyHostToDevice));
  G2S_HIP_TRY(d_kown.alloc(((size_t)nruns + 1) * 4));
  G2S_HIP_TRY(d_pown.alloc(((size_t)nruns + 1) * 4));
  G2S_HIP_TRY(d_ksh.alloc(((size_t)FU + 1) * 4));
  G2S_HIP_TRY(d_psh.alloc(((size_t)FU + 1) * 4));
  hipLaunchKernelGGL(k_pool_keep_own<KT>, grid((uint64_t)nruns + 1), blk, 0, 0, (const KT*)d_rkey.p, (const uint32_t*)d_rset.p,
                     (const uint32_t*)d_rcnt.p, nruns, (const uint32_t*)d_sf.p, (const KT*)d_hkey.p, U, so, (uint32_t*)d_kown.p);
  if (FU) {
    hipLaunchKernelGGL(k_pool_keep_shared<KT>, grid((uint64_t)FU + 1), blk, 0, 0, (const KT*)d_hkey.p, (const uint32_t*)d_hcnt.p, U,
                       (const uint32_t*)d_fset.p, FU, (const uint32_t*)d_rlo.p, (const KT*)d_rkey.p, (const uint32_t*)d_rcnt.p, so,
                       (uint32_t*)d_ksh.p);
  } else {
    G2S_HIP_TRY(hipMemset(d_ksh.p, 0, 4));
  }
  G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_kown.p, (uint32_t*)d_pown.p, (size_t)nruns + 1));
  G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_ksh.p, (uint32_t*)d_psh.p, (size_t)FU + 1));
  G2S_HIP_TRY(d_cnt.alloc(((size_t)nsets + 1) * 4));
  G2S_HIP_TRY(d_base.alloc(((size_t)nsets + 1) * 4));
  hipLaunchKernelGGL(k_pool_set_count, grid((uint64_t)nsets + 1), blk, 0, 0, (const uint32_t*)d_rlo.p, (const uint32_t*)d_pown.p,
                     (const uint32_t*)d_sf.p, (const uint32_t*)d_psh.p, U, nsets, (uint32_t*)d_cnt.p);
  G2S_HIP_TRY(exclusive_scan((const uint32_t*)d_cnt.p, (uint32_t*)d_base.p, (size_t)nsets + 1));
  std::vector<uint32_t> lo32((size_t)nsets + 1, 0);
  G2S_HIP_TRY(hipMemcpy(lo32.data(), d_base.p, lo32.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t n_solid = lo32[nsets];
  std::vector<KT> host((size_t)n_solid);
  std::vector<uint32_t> rs((size_t)n_solid);
  if (n_solid) {
    G2S_HIP_TRY(d_out.alloc((size_t)n_solid * sizeof(KT)));
    G2S_HIP_TRY(d_osid.alloc((size_t)n_solid * 4));
    if (nruns) {
      hipLaunchKernelGGL(k_pool_write_own<KT>, grid(nruns), blk, 0, 0, (const KT*)d_rkey.p, (const uint32_t*)d_rset.p, nruns,
                         (const uint32_t*)d_kown.p, (const uint32_t*)d_pown.p, (const uint32_t*)d_rlo.p, (const uint32_t*)d_sf.p,
                         (const KT*)d_hkey.p, U, (const uint32_t*)d_psh.p, (const uint32_t*)d_base.p, (KT*)d_out.p, (uint32_t*)d_osid.p);
    }
    if (FU) {
      hipLaunchKernelGGL(k_pool_write_shared<KT>, grid(FU), blk, 0, 0, (const KT*)d_hkey.p, U, (const uint32_t*)d_fset.p, FU,
                         (const uint32_t*)d_ksh.p, (const uint32_t*)d_psh.p, (const uint32_t*)d_rlo.p, (const KT*)d_rkey.p,
                         (const uint32_t*)d_pown.p, (const uint32_t*)d_base.p, (KT*)d_out.p, (uint32_t*)d_osid.p);
    }
    G2S_HIP_TRY(hipMemcpy(host.data(), d_out.p, (size_t)n_solid * sizeof(KT), hipMemcpyDeviceToHost));
    G2S_HIP_TRY(hipMemcpy(rs.data(), d_osid.p, (size_t)n_solid * 4, hipMemcpyDeviceToHost));
  }
  G2S_HIP_TRY(hipGetLastError());
  out.swap(host);
  rank_set->swap(rs);
  g.n = n_solid;
  g.set_lo.assign(lo32.begin(), lo32.end());
  return true;
}

bool graph_build_pool_gpu(Graph& g, const PoolSets& ps, int solid, int device,
                          const std::function<void(const std::vector<uint32_t>&, uint32_t)>& host_walk, PoolBuildInfo* info,
                          std::string* why, const PoolReach* reach, PoolReachInfo* rinfo, bool* device_usable) {
  if (device_usable) *device_usable = false;
  return with_kmer_type(g.kmer_bytes, [&](auto t) {
    using KT = typename decltype(t)::type;
    std::vector<uint32_t> rank_set;
    return count_solid_pool_gpu_t<KT>(g, &rank_set, ps, solid, device, info, why, reach, rinfo, device_usable) &&
           finish_gpu_t<KT>(g, device, host_walk, why, &rank_set);
  });
}

}  // namespace g2s

#include "solid_passes.h"

namespace g2s {

bool count_solid_gpu(Graph& g, const BuildInput& in, int solid, int device, std::string* why, SolidCountInfo* info) {
  return with_kmer_type(g.kmer_bytes, [&](auto t) {
    return count_solid_gpu_t<typename decltype(t)::type>(g, in, solid, device, why, info);
  });
}

bool graph_finish_gpu(Graph& g, int device, const std::function<void(const std::vector<uint32_t>&, uint32_t)>& host_walk,
                      std::string* why) {
  return with_kmer_type(g.kmer_bytes, [&](auto t) {
    return finish_gpu_t<typename decltype(t)::type>(g, device, host_walk, why);
  });
}

}  // namespace g2s
