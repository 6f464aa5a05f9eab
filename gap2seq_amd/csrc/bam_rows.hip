// gap2seq_amd/csrc/bam_rows.hip — pass A of the batched read filter on the GPU: from an inflated window in device
// memory to the rows of its records (bam_rows.h), without the host walking the file.
//
// A record's start is known only from the size field of the record before it, so a window is walked in four steps,
// every one a launch on the reader's stream behind the inflate kernel, none of them waiting for another workgroup:
//   candidates  k_flag       every offset of the window whose 36 bytes could be a record's head: what BamFile::for_each
//                            enforces (32 <= block_size <= 2^30, l_seq >= 0, l_name != 0, the layout within block_size)
//                            and what the format adds (the name's last byte is NUL, ref_id and next_ref_id in
//                            [-1, n_ref), pos >= -1).  Tiles of 4 096 offsets staged in LDS with a halo of 36 bytes;
//                            counted per tile, scanned by one workgroup (k_scan), written in offset order by ballot.
//                            Slot 0 of the list is the chain's head, handed over by the window before.
//   links       k_links      candidate c points to the candidate at c + 4 + block_size(c) (binary search); DEAD when
//                            there is none; EXIT when that offset's head does not fit before the window's end (c is a
//                            whole record and the chain leaves at that offset) or c itself ends beyond it (the chain
//                            leaves at c)
//   chain       k_round      pointer doubling with marks: marked = {head}; every round each marked candidate marks
//                            J[c], then J <- J o J (two buffers).  After ceil(log2(capacity)) rounds, a number fixed by
//                            the window's size, the marked candidates are the records the host walk would visit.
//   rows        k_rec        the chain rises in offset, so a record's index in the window is the exclusive scan of the
//                            marks (count per workgroup, k_scan, ballot); one thread a record reads the fixed fields,
//                            sums the CIGAR as BamRec::end_pos does and hashes both names (name_hash.h)
// The read route's streaming form (bam_reads.h) asks for compact rows instead: k_rec_compact writes a record's offset
// in the window buffer and its flag to a ring of the walk window's capacity, and the caller's sink consumes the ring
// behind it on the same stream — no array grows with the file, and the row limit of 2^32 does not apply.
// From window to window the chain's EXIT offset stays in the control block (State::head), and the bytes from there to the
// window's end are copied in front of the next window's buffer (k_carry).  Whatever does not fit this scheme — a marked
// candidate with a DEAD link, more candidates than the capacity, a carry longer than the room in front, a chain that
// does not end at the stream's end — sets State::anomaly, after which every kernel returns at once: the caller throws
// the rows away and the host walk, which is the authority on what is wrong with a file, runs instead.
// Every index is checked against its array's capacity before a write.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>

#include "bam_rows.h"
#include "hip_host.h"
#include "name_hash.h"
#include "readfilter_gaps.hpp"

namespace {

constexpr uint32_t kBlock = 256, kWave = 64, kWaves = kBlock / kWave;
constexpr uint32_t kTile = 4096;  // offsets a workgroup flags
constexpr uint32_t kHead = 36;    // block_size and the 32 fixed bytes
constexpr uint32_t kIters = kTile / kBlock;
constexpr uint32_t kDead = 0xFFFFFFFFu, kExit = 0xFFFFFFFEu;
constexpr uint32_t kSlack = 64;   // candidates a window may hold beyond one per 36 bytes and its head
constexpr uint32_t kScan = 1024;

struct State {
  int32_t head;       // offset of the chain's head, relative to the current window's first byte (negative: carried)
  int32_t exit;       // where this walk window's chain leaves it
  uint32_t n_cand;    // candidates of this walk window, the head included
  uint32_t n_rec;     // its records
  uint32_t anomaly;   // g2s::RowsAnomaly
  int32_t read_length;
  uint32_t dead;      // a marked candidate of this walk window has a DEAD link: k_scan<1> makes it the anomaly
  uint32_t pad_;
  uint64_t base;      // rows of the windows before
  uint64_t row_base;  // where this walk window's rows go
  uint64_t max_span;
  uint64_t candidates;
};

struct RecHead {
  uint32_t w[9];  // block_size, ref_id, pos, l_name | mapq << 8 | bin << 16, n_cigar | flag << 16, l_seq, next_ref_id, ..
};

__device__ __forceinline__ uint32_t g_ld32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
__device__ __forceinline__ uint32_t lds_ld32(const uint32_t* words, uint32_t byte) {
  const uint32_t w0 = words[byte >> 2], sh = (byte & 3u) * 8u;
  return sh ? (w0 >> sh | words[(byte >> 2) + 1] << (32u - sh)) : w0;
}

__device__ __forceinline__ bool plausible(const RecHead& h, int32_t n_ref) {
  const uint32_t bs = h.w[0];
  if (bs < 32u || bs > (1u << 30)) return false;
  const int32_t ref = (int32_t)h.w[1], pos = (int32_t)h.w[2], l_seq = (int32_t)h.w[5], next_ref = (int32_t)h.w[6];
  const uint32_t l_name = h.w[3] & 0xFFu, n_cigar = h.w[4] & 0xFFFFu;
  if (l_seq < 0 || l_name == 0) return false;
  if (32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > bs) return false;
  return ref >= -1 && ref < n_ref && next_ref >= -1 && next_ref < n_ref && pos >= -1;
}
// the name's last byte, when the window holds it
__device__ __forceinline__ bool name_ends(const uint8_t* win, int32_t o, uint32_t l_name, int32_t wend) {
  const int64_t p = (int64_t)o + kHead + l_name - 1;
  return p >= wend || win[p] == 0;
}

// WRITE false: blk[tile] = the candidates among the tile's offsets; WRITE true: their offsets at cand[1 + blk[tile] ...]
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) k_flag(const uint8_t* __restrict__ win, const State* __restrict__ st, int32_t wstart,
                                                 int32_t wend, int32_t n_ref, uint32_t cap, uint32_t* __restrict__ blk,
                                                 int32_t* __restrict__ cand) {
  __shared__ uint32_t tile[kTile / 4 + 12];
  __shared__ uint32_t wave_cnt[kWaves];
  if (st->anomaly) return;
  const uint32_t tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int32_t tile_beg = wstart + (int32_t)(blockIdx.x * kTile);
  if (tile_beg >= wend) {
    if (!WRITE && tid == 0) blk[blockIdx.x] = 0;
    return;
  }
  const int32_t tile_end = tile_beg + (int32_t)kTile < wend ? tile_beg + (int32_t)kTile : wend;
  const int32_t lo = tile_beg & ~3;  // (the window's first byte is word aligned)
  const uint32_t nwords = (uint32_t)(tile_end + (int32_t)kHead - lo + 3) / 4u;  // at most kTile / 4 + 11
  const uint32_t* src = (const uint32_t*)(win + lo);
  for (uint32_t i = tid; i < nwords; i += kBlock) tile[i] = src[i];
  __syncthreads();
  const int32_t head = st->head;
  uint64_t m[kIters];
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t it = 0; it < kIters; it++) {
    const int32_t o = tile_beg + (int32_t)(wave * (kTile / kWaves) + it * kWave + lane);
    bool f = false;
    if (o < tile_end && o + (int32_t)kHead <= wend && o != head) {
      RecHead h;
      const uint32_t b = (uint32_t)(o - lo);
#pragma unroll
      for (uint32_t k = 0; k < 9; k++) h.w[k] = lds_ld32(tile, b + 4u * k);
      f = plausible(h, n_ref) && name_ends(win, o, h.w[3] & 0xFFu, wend);
    }
    m[it] = __ballot(f);
    cnt += (uint32_t)__popcll(m[it]);
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (!WRITE) {
    if (tid == 0) blk[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return;
  }
  uint32_t at = 1u + blk[blockIdx.x];
  for (uint32_t w = 0; w < wave; w++) at += wave_cnt[w];
#pragma unroll
  for (uint32_t it = 0; it < kIters; it++) {
    if (m[it] >> lane & 1u) {
      const uint32_t idx = at + (uint32_t)__popcll(m[it] & (((uint64_t)1 << lane) - 1));
      if (idx < cap) cand[idx] = tile_beg + (int32_t)(wave * (kTile / kWaves) + it * kWave + lane);
    }
    at += (uint32_t)__popcll(m[it]);
  }
}

// One workgroup: blk[0 .. n) from counts to their exclusive scan.  WHICH 0 (candidates): the list's size against its
// capacity, its slot 0.  WHICH 1 (records): where the window's rows go, and the head of the window that follows.
// (rows_over: the anomaly of rows beyond cap_rows — the kernels' limits, or in store form a planned count)
template <int WHICH>
__global__ void __launch_bounds__(kScan) k_scan(uint32_t* __restrict__ blk, uint32_t n, State* __restrict__ st, uint32_t cap_cand,
                                                uint64_t cap_rows, int32_t* __restrict__ cand, uint32_t rows_over) {
  __shared__ uint32_t part[kScan];
  if (st->anomaly) return;
  const uint32_t tid = threadIdx.x, per = (n + kScan - 1) / kScan;
  const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += blk[i];
  part[tid] = s;
  __syncthreads();
  for (uint32_t off = 1; off < kScan; off <<= 1) {
    const uint32_t v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - s;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t c = blk[i];
    blk[i] = run;
    run += c;
  }
  if (tid != kScan - 1) return;
  const uint32_t total = part[kScan - 1];
  if (WHICH == 0) {
    if (total + 1u > cap_cand) {
      st->anomaly = g2s::kRowsOverflow;
      st->n_cand = 0;
    } else {
      st->n_cand = total + 1u;
      cand[0] = st->head;
      st->exit = INT32_MIN;
      st->dead = 0;
    }
  } else {
    if (st->dead || st->exit == INT32_MIN) {
      st->anomaly = g2s::kRowsDeadLink;
    } else if (st->base + total > cap_rows) {
      st->anomaly = rows_over;
    } else {
      st->row_base = st->base;
      st->n_rec = total;
      st->base += total;
      st->candidates += st->n_cand;
      st->head = st->exit;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_links(const uint8_t* __restrict__ win, const State* __restrict__ st, int32_t wend,
                                                  int32_t n_ref, const int32_t* __restrict__ cand, uint32_t* __restrict__ link,
                                                  uint32_t* __restrict__ j0, uint8_t* __restrict__ mark, uint8_t* __restrict__ emit) {
  if (st->anomaly) return;
  const uint32_t n = st->n_cand, i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cand[i];
  uint32_t L = kDead;
  uint8_t e = 0;
  if ((int64_t)c + kHead > wend) {
    L = kExit;  // (the head alone: its own 36 bytes are not all here yet)
  } else {
    RecHead h;
    for (uint32_t k = 0; k < 9; k++) h.w[k] = g_ld32(win + c + 4 * (int32_t)k);
    if (i != 0 || (plausible(h, n_ref) && name_ends(win, c, h.w[3] & 0xFFu, wend))) {
      const int64_t t = (int64_t)c + 4 + h.w[0];
      if (t > wend) {
        L = kExit;
      } else {
        e = 1;
        if (t + kHead > wend) {
          L = kExit;
        } else {
          uint32_t lo = 0, hi = n;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cand[mid] < t) lo = mid + 1; else hi = mid;
          }
          if (lo < n && cand[lo] == t) L = lo;
        }
      }
    }
  }
  link[i] = L;
  j0[i] = L;
  mark[i] = i == 0;
  emit[i] = e;
}

// (a mark set in this round may or may not be seen by its own candidate in this round: either way the marked are
// candidates of the chain, and after r rounds they include its first 2^r)
__global__ void __launch_bounds__(kBlock) k_round(const State* __restrict__ st, const uint32_t* __restrict__ jin,
                                                  uint32_t* __restrict__ jout, uint8_t* mark) {
  if (st->anomaly) return;
  const uint32_t n = st->n_cand, i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = jin[i];
  if (j < n) {
    if (mark[i]) mark[j] = 1;
    jout[i] = jin[j];
  } else {
    jout[i] = j;
  }
}

__device__ __forceinline__ void make_row(const uint8_t* __restrict__ rec, uint64_t row, State* st, int32_t* __restrict__ ref_id,
                                         int32_t* __restrict__ pos_out, int64_t* __restrict__ end_out, uint32_t* __restrict__ flag_out,
                                         uint64_t* __restrict__ h_own, uint64_t* __restrict__ h_mate,
                                         uint64_t* __restrict__ rec_off, uint64_t off) {
  const uint8_t* p = rec + 4;
  const int32_t ref = (int32_t)g_ld32(p), pos = (int32_t)g_ld32(p + 4), l_seq = (int32_t)g_ld32(p + 16);
  const uint32_t l_name = p[8], w = g_ld32(p + 12), n_cigar = w & 0xFFFFu, flag = w >> 16;
  int64_t rlen = 0;
  if (!(flag & g2s::BAM_UNMAPPED)) {
    const uint8_t* cg = p + 32 + l_name;
    for (uint32_t i = 0; i < n_cigar; i++) {
      const uint32_t c = g_ld32(cg + 4 * (size_t)i), op = c & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;  // M D N = X
    }
  }
  const int64_t end = (int64_t)pos + (rlen ? rlen : 1);
  const uint8_t* name = p + 32;
  uint32_t n = 0;
  while (n < l_name && name[n]) n++;
  const uint32_t own = (flag & g2s::BAM_READ1) ? 1u : 2u;
  ref_id[row] = ref;
  pos_out[row] = pos;
  end_out[row] = end;
  flag_out[row] = flag;
  h_own[row] = g2s::name_hash(name, n, own);
  h_mate[row] = g2s::name_hash(name, n, 3u - own);
  if (rec_off) rec_off[row] = off;  // (one-pass mode: where pass B finds the record in the resident stream)
  if (l_seq > st->read_length) atomicMax(&st->read_length, l_seq);
  if (ref >= 0) {
    const uint64_t span = (uint64_t)(end - (int64_t)pos);
    if (span > st->max_span) atomicMax((unsigned long long*)&st->max_span, (unsigned long long)span);
  }
}

// a whole record's index among its walk window's, from the scan of the workgroups' counts and the ballot of its wave
// (wave_cnt: the workgroup's four wave counts, behind its barrier)
__device__ __forceinline__ uint32_t rec_rank(const uint32_t* __restrict__ blk, const uint32_t* wave_cnt, uint64_t mask, uint32_t wave,
                                             uint32_t lane) {
  uint32_t rank = blk[blockIdx.x] + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
  for (uint32_t w = 0; w < wave; w++) rank += wave_cnt[w];
  return rank;
}

// WRITE false: blk[workgroup] = the marked candidates that are whole records; the chain's way out of the window, or
// its dead end (State::dead, not the anomaly word itself: every wave of this launch has to pass the test at the
// kernel's entry the same way, or a workgroup's waves would part in front of its barrier).  WRITE true: their rows.
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) k_rec(const uint8_t* __restrict__ win, State* st, const int32_t* __restrict__ cand,
                                                const uint32_t* __restrict__ link, const uint8_t* __restrict__ mark,
                                                const uint8_t* __restrict__ emit, uint32_t* __restrict__ blk, int32_t* ref_id,
                                                int32_t* pos, int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate,
                                                uint64_t* rec_off, uint64_t win_off) {
  __shared__ uint32_t wave_cnt[kWaves];
  if (st->anomaly) return;
  const uint32_t n = st->n_cand, tid = threadIdx.x, i = blockIdx.x * kBlock + tid, wave = tid / kWave, lane = tid % kWave;
  const bool marked = i < n && mark[i];
  const bool take = marked && emit[i];
  if (!WRITE && marked) {
    const uint32_t L = link[i];
    if (L == kDead) st->dead = 1;
    else if (L == kExit) st->exit = take ? (int32_t)((int64_t)cand[i] + 4 + g_ld32(win + cand[i])) : cand[i];
  }
  const uint64_t mask = __ballot(take);
  if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!WRITE) {
    if (tid == 0) blk[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return;
  }
  if (!take) return;
  const uint32_t rank = rec_rank(blk, wave_cnt, mask, wave, lane);
  make_row(win + cand[i], st->row_base + rank, st, ref_id, pos, end, flag, h_own, h_mate, rec_off,
           (uint64_t)((int64_t)win_off + (int64_t)cand[i]));
}

// k_rec<true> for the compact form: of every whole record its offset in the window buffer and its flag, at its index in
// this walk window, in the ring
__global__ void __launch_bounds__(kBlock) k_rec_compact(const uint8_t* __restrict__ win, const State* __restrict__ st,
                                                        const int32_t* __restrict__ cand, const uint8_t* __restrict__ mark,
                                                        const uint8_t* __restrict__ emit, const uint32_t* __restrict__ blk,
                                                        int32_t* __restrict__ ring_off, uint32_t* __restrict__ ring_flag,
                                                        uint32_t ring_cap) {
  __shared__ uint32_t wave_cnt[kWaves];
  if (st->anomaly) return;
  const uint32_t n = st->n_cand, tid = threadIdx.x, i = blockIdx.x * kBlock + tid, wave = tid / kWave, lane = tid % kWave;
  const bool take = i < n && mark[i] && emit[i];
  const uint64_t mask = __ballot(take);
  if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!take) return;
  const uint32_t rank = rec_rank(blk, wave_cnt, mask, wave, lane);
  if (rank < ring_cap) {
    ring_off[rank] = cand[i];
    ring_flag[rank] = g_ld32(win + cand[i] + 16) >> 16;
  }
}

// the bytes from the chain's exit to the window's end, in front of the next window's buffer
__global__ void __launch_bounds__(kBlock) k_carry(const uint8_t* __restrict__ win, int64_t bytes, uint8_t* __restrict__ next_win,
                                                  int64_t front, State* st) {
  if (st->anomaly) return;
  const int64_t carry = bytes - (int64_t)st->head;
  const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;
  if (carry < 0 || carry > front) {
    if (gid == 0) st->anomaly = g2s::kRowsCarry;
    return;
  }
  const uint8_t* src = win + st->head;
  uint8_t* dst = next_win - carry;
  for (int64_t i = gid; i < carry; i += (int64_t)gridDim.x * kBlock) dst[i] = src[i];
}
// the same step in a resident stream, where the window that follows lies behind this one and the cut record is whole
// in memory already: the room in front is checked as k_carry checks it (so that a file is handed over to the host walk
// in either mode or in neither), nothing is copied, and the head moves by the distance between the windows' bases
__global__ void k_advance(State* st, int64_t win_end, int64_t step, int64_t front) {
  if (st->anomaly) return;
  const int64_t carry = win_end - (int64_t)st->head;
  if (carry < 0 || carry > front) {
    st->anomaly = g2s::kRowsCarry;
    return;
  }
  st->head = (int32_t)((int64_t)st->head - step);
}
__global__ void k_rebase(State* st, int64_t bytes) {
  if (!st->anomaly) st->head = (int32_t)((int64_t)st->head - bytes);
}
__global__ void k_end(State* st, int64_t bytes) {
  if (!st->anomaly && (int64_t)st->head != bytes) st->anomaly = g2s::kRowsWrongEnd;
}

uint32_t window_capacity(size_t bytes) { return (uint32_t)(bytes / kHead) + kSlack + 1u; }

}  // namespace

namespace g2s {

// the object's device allocations: freed by their destructors, the last declared first
struct BamRowsDevice::Buffers {
  DevMem stream_buf, rec_off, h_mate, h_own, flag, end, pos, ref_id, ring_flag, ring_off, blk, emit, mark, j1, j0, link, cand, state;
};

BamRowsDevice* BamRowsDevice::create(int device, void* stream, size_t max_window, size_t walk_window, size_t front,
                                     uint64_t cap_rows, int32_t n_ref, uint64_t first_head, std::string* why,
                                     const ResidentAsk* ask, int* resident_refused, const RowsSink* sink) {
  const size_t walk = walk_window && walk_window < max_window ? walk_window : (max_window ? max_window : 1);
  const bool compact = sink != nullptr;
  if (compact) cap_rows = UINT64_MAX;  // (a walk window's rows are bounded by its candidates)
  // (store form: the row limit applies to the planned rows, which replace cap_rows below)
  const bool may_store = !compact && ask && ask->bytes && ask->store != 0 && ask->plan;
  bool whole_rows = compact || cap_rows < (uint64_t)UINT32_MAX - 1;
  if (max_window + front + 64 >= (size_t)INT32_MAX || first_head > max_window || (!whole_rows && !may_store) ||
      (compact && ask && ask->bytes)) {
    if (why) *why = "a file outside the row kernels' index widths";
    return nullptr;
  }
  BamRowsDevice* D = new BamRowsDevice();
  Buffers& B = *(D->buf_ = new Buffers());
  D->device_ = device;
  D->stream_ = stream;
  D->walk_ = walk;
  D->front_ = front;
  D->cap_rows_ = cap_rows;
  D->n_ref_ = n_ref;
  D->compact_ = compact;
  if (compact) D->sink_ = *sink;
  D->cap_cand_ = window_capacity(walk);
  D->max_tiles_ = (uint32_t)((walk + kTile - 1) / kTile);
  const size_t nblk = std::max<size_t>(D->max_tiles_, (D->cap_cand_ + kBlock - 1) / kBlock) + 1;
  auto make = [&]() -> bool {
    size_t rows = compact ? 0 : (size_t)cap_rows + 1;
    const size_t cc = D->cap_cand_;
    G2S_HIP_TRY(hipSetDevice(device));
    // one-pass mode: the whole inflated stream and the records' offsets, when they fit under the cap with the rows
    if (ask && ask->bytes) {
      size_t free_b = 0, total_b = 0;
      G2S_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      const uint64_t need = ask->bytes + 64 + rows * 52, cap = std::min<uint64_t>(free_b / 2, ask->cap ? ask->cap : UINT64_MAX);
      const bool forced = may_store && ask->store > 0;
      if (forced || need > cap || !whole_rows) {  // (forced: the whole stream is not tried)
        *resident_refused = kResidentOverCap;
      } else {
        DevMem off, buf;  // (taken buf first; when either fails, freed buf first, before anything else is taken)
        if (buf.alloc((size_t)ask->bytes + 64) != hipSuccess || off.alloc(rows * 8) != hipSuccess) {
          (void)hipGetLastError();
          *resident_refused = kResidentNoMemory;
        } else {
          D->stream_buf_ = (B.stream_buf = std::move(buf)).as<uint8_t>();
          D->rows_.rec_off = (B.rec_off = std::move(off)).as<uint64_t>();
          D->stream_bytes_ = ask->bytes;
        }
      }
      // the store route: the whole stream is over the cap (or the caller insists), and the planned store and rows fit it
      if (may_store && (forced || *resident_refused == kResidentOverCap)) {
        StorePlan plan;
        *resident_refused = kResidentOverCap;
        if (ask->plan(&plan) && plan.rows_cap < (uint64_t)UINT32_MAX - 1 && plan.need <= cap) {
          StoreReport& rep = D->report_;
          rep.store_cap = plan.store_cap, rep.rows_cap = plan.rows_cap, rep.device_bytes = plan.need;
          std::string w;
          DevMem off;
          D->store_ = BamStoreDevice::create(device, stream, plan.store_cap, plan.rows_cap, D->cap_cand_, &w);
          if (!D->store_ || off.alloc(((size_t)plan.rows_cap + 1) * 8) != hipSuccess) {
            (void)hipGetLastError();
            delete D->store_;
            D->store_ = nullptr;
            *resident_refused = kResidentNoMemory;
          } else {
            D->cap_rows_ = cap_rows = plan.rows_cap;
            rows = (size_t)cap_rows + 1;
            whole_rows = true;
            D->stream_buf_ = D->store_->buffer();
            D->rows_.rec_off = (B.rec_off = std::move(off)).as<uint64_t>();
            *resident_refused = kResidentKept;
          }
        }
      }
    }
    if (!whole_rows) {
      if (why) *why = "a file outside the row kernels' index widths";
      return false;
    }
    uint64_t held = 0;  // what the allocations below ask for
    auto take = [&held](DevMem& m, size_t bytes) {
      held += bytes ? bytes : 16;
      return m.alloc(bytes);
    };
    G2S_HIP_TRY(take(B.state, sizeof(State)));
    G2S_HIP_TRY(take(B.cand, cc * 4));
    G2S_HIP_TRY(take(B.link, cc * 4));
    G2S_HIP_TRY(take(B.j0, cc * 4));
    G2S_HIP_TRY(take(B.j1, cc * 4));
    G2S_HIP_TRY(take(B.mark, cc));
    G2S_HIP_TRY(take(B.emit, cc));
    G2S_HIP_TRY(take(B.blk, nblk * 4));
    if (compact) {
      G2S_HIP_TRY(take(B.ring_off, cc * 4));
      G2S_HIP_TRY(take(B.ring_flag, cc * 4));
    }
    G2S_HIP_TRY(take(B.ref_id, rows * 4));
    G2S_HIP_TRY(take(B.pos, rows * 4));
    G2S_HIP_TRY(take(B.end, rows * 8));
    G2S_HIP_TRY(take(B.flag, rows * 4));
    G2S_HIP_TRY(take(B.h_own, rows * 8));
    G2S_HIP_TRY(take(B.h_mate, rows * 8));
    if (compact && held != compact_bytes(walk)) {  // (what the streaming form counted against its limit)
      if (why) *why = "the compact form's allocations are not what compact_bytes() says";
      return false;
    }
    DeviceRows& R = D->rows_;  // (the plain pointers the joins read)
    R.ref_id = B.ref_id.as<int32_t>(), R.pos = B.pos.as<int32_t>(), R.end = B.end.as<int64_t>(), R.flag = B.flag.as<uint32_t>();
    R.h_own = B.h_own.as<uint64_t>(), R.h_mate = B.h_mate.as<uint64_t>();
    State s{};
    s.head = (int32_t)first_head;
    s.max_span = 1;
    G2S_HIP_TRY(hipMemcpyAsync(B.state.p, &s, sizeof s, hipMemcpyHostToDevice, (hipStream_t)stream));
    G2S_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // (`s` leaves scope)
    return true;
  };
  if (!make()) {
    delete D;
    return nullptr;
  }
  return D;
}

uint32_t BamRowsDevice::ring_capacity_of(size_t walk_window) { return window_capacity(walk_window ? walk_window : 1); }

uint64_t BamRowsDevice::compact_bytes(size_t walk_window) {
  const uint64_t cc = window_capacity(walk_window ? walk_window : 1), tiles = (walk_window + kTile - 1) / kTile;
  const uint64_t nblk = std::max<uint64_t>(tiles, (cc + kBlock - 1) / kBlock) + 1;
  // (cand, link, j0, j1, the ring's two arrays; mark, emit; blk; the control block; the six empty row arrays)
  return cc * (6 * 4 + 2) + nblk * 4 + sizeof(State) + 6 * 16;
}

BamRowsDevice::~BamRowsDevice() {
  if (device_ >= 0) (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
  delete store_;
  delete buf_;  // (the allocations free themselves)
}

bool BamRowsDevice::window(const uint8_t* d_win, size_t start, size_t bytes, std::string* why, uint64_t win_off) {
  hipStream_t s = (hipStream_t)stream_;
  State* st = buf_->state.as<State>();
  int32_t* cand = buf_->cand.as<int32_t>();
  uint32_t *link = buf_->link.as<uint32_t>(), *blk = buf_->blk.as<uint32_t>();
  uint8_t *mark = buf_->mark.as<uint8_t>(), *emit = buf_->emit.as<uint8_t>();
  G2S_HIP_TRY(hipSetDevice(device_));
  const uint32_t rows_over = store_ ? (uint32_t)kRowsPlanRows : (uint32_t)kRowsLimits;
  for (size_t ws = start; ws < bytes; ws += walk_) {
    const size_t we = std::min(ws + walk_, bytes);
    const uint32_t cap = window_capacity(we - ws);  // (at most cap_cand_)
    const uint32_t tiles = (uint32_t)((we - ws + kTile - 1) / kTile), groups = (cap + kBlock - 1) / kBlock;
    uint32_t rounds = 0;
    while (((uint32_t)1 << rounds) < cap) rounds++;
    hipLaunchKernelGGL((k_flag<false>), dim3(tiles), dim3(kBlock), 0, s, d_win, (const State*)st, (int32_t)ws, (int32_t)we, n_ref_,
                       cap, blk, cand);
    hipLaunchKernelGGL((k_scan<0>), dim3(1), dim3(kScan), 0, s, blk, tiles, st, cap, cap_rows_, cand, rows_over);
    hipLaunchKernelGGL((k_flag<true>), dim3(tiles), dim3(kBlock), 0, s, d_win, (const State*)st, (int32_t)ws, (int32_t)we, n_ref_,
                       cap, blk, cand);
    hipLaunchKernelGGL(k_links, dim3(groups), dim3(kBlock), 0, s, d_win, (const State*)st, (int32_t)we, n_ref_,
                       (const int32_t*)cand, link, buf_->j0.as<uint32_t>(), mark, emit);
    uint32_t *jin = buf_->j0.as<uint32_t>(), *jout = buf_->j1.as<uint32_t>();
    for (uint32_t r = 0; r < rounds; r++) {
      hipLaunchKernelGGL(k_round, dim3(groups), dim3(kBlock), 0, s, (const State*)st, (const uint32_t*)jin, jout, mark);
      std::swap(jin, jout);
    }
    hipLaunchKernelGGL((k_rec<false>), dim3(groups), dim3(kBlock), 0, s, d_win, st, (const int32_t*)cand, (const uint32_t*)link,
                       (const uint8_t*)mark, (const uint8_t*)emit, blk, rows_.ref_id, rows_.pos, rows_.end, rows_.flag, rows_.h_own,
                       rows_.h_mate, rows_.rec_off, win_off);
    hipLaunchKernelGGL((k_scan<1>), dim3(1), dim3(kScan), 0, s, blk, groups, st, cap, cap_rows_, cand, rows_over);
    int32_t* ring_off = buf_->ring_off.as<int32_t>();
    uint32_t* ring_flag = buf_->ring_flag.as<uint32_t>();
    if (compact_)
      hipLaunchKernelGGL(k_rec_compact, dim3(groups), dim3(kBlock), 0, s, d_win, (const State*)st, (const int32_t*)cand,
                         (const uint8_t*)mark, (const uint8_t*)emit, (const uint32_t*)blk, ring_off, ring_flag, cap_cand_);
    else
      hipLaunchKernelGGL((k_rec<true>), dim3(groups), dim3(kBlock), 0, s, d_win, st, (const int32_t*)cand, (const uint32_t*)link,
                         (const uint8_t*)mark, (const uint8_t*)emit, blk, rows_.ref_id, rows_.pos, rows_.end, rows_.flag, rows_.h_own,
                         rows_.h_mate, rows_.rec_off, win_off);
    G2S_HIP_TRY(hipGetLastError());
    // store form: rec_off holds the offsets in this window (win_off is 0), and the store's kernels replace them
    if (store_ && !store_->window(d_win, front_, we, &st->n_rec, &st->row_base, &st->anomaly, rows_.rec_off, why)) return false;
    if (compact_) {
      CompactRows cr;
      cr.off = ring_off, cr.flag = ring_flag, cr.n_rec = &st->n_rec, cr.anomaly = &st->anomaly, cr.capacity = cap_cand_, cr.stream = stream_;
      if (!sink_(cr, d_win, front_, we, why)) return false;
    }
    windows_++;
  }
  return true;
}

bool BamRowsDevice::carry(const uint8_t* d_win, size_t bytes, uint8_t* d_next_win, std::string* why) {
  hipStream_t s = (hipStream_t)stream_;
  G2S_HIP_TRY(hipSetDevice(device_));
  hipLaunchKernelGGL(k_carry, dim3(64), dim3(kBlock), 0, s, d_win, (int64_t)bytes, d_next_win, (int64_t)front_, buf_->state.as<State>());
  hipLaunchKernelGGL(k_rebase, dim3(1), dim3(1), 0, s, buf_->state.as<State>(), (int64_t)bytes);
  G2S_HIP_TRY(hipGetLastError());
  return true;
}

bool BamRowsDevice::advance(size_t win_end, size_t step, std::string* why) {
  hipStream_t s = (hipStream_t)stream_;
  G2S_HIP_TRY(hipSetDevice(device_));
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, buf_->state.as<State>(), (int64_t)win_end, (int64_t)step, (int64_t)front_);
  G2S_HIP_TRY(hipGetLastError());
  return true;
}

bool BamRowsDevice::finish(size_t last_bytes, int* anomaly, std::string* why) {
  hipStream_t s = (hipStream_t)stream_;
  G2S_HIP_TRY(hipSetDevice(device_));
  hipLaunchKernelGGL(k_end, dim3(1), dim3(1), 0, s, buf_->state.as<State>(), (int64_t)last_bytes);
  G2S_HIP_TRY(hipGetLastError());
  State h{};
  G2S_HIP_TRY(hipMemcpyAsync(&h, buf_->state.p, sizeof h, hipMemcpyDeviceToHost, s));
  G2S_HIP_TRY(hipStreamSynchronize(s));
  *anomaly = (int)h.anomaly;
  rows_.n = h.base;
  rows_.max_span = (int64_t)h.max_span;
  rows_.read_length = h.read_length;
  candidates_ = h.candidates;
  if (store_) {  // the store's position and words, once
    bool over = false, bad = false;
    if (!store_->finish(&report_.store_bytes, &report_.records, &over, &bad, why)) return false;
    stream_bytes_ = report_.store_bytes;
    if (h.anomaly == kRowsPlanRows) report_.overflow = 1;
    else if (h.anomaly == kRowsOk && bad) *anomaly = kRowsDeadLink;  // (a record outside its window: the host walk decides)
    else if (h.anomaly == kRowsOk && over) *anomaly = kRowsPlanStore, report_.overflow = 2;
    report_.used = *anomaly == kRowsOk ? 1 : 0;
  }
  return true;
}

bool BamRowsDevice::download(uint64_t m, int32_t* ref_id, int32_t* pos, int64_t* end, uint32_t* flag, uint64_t* h_own,
                             uint64_t* h_mate, std::string* why) const {
  if (!m) return true;
  G2S_HIP_TRY(hipSetDevice(device_));
  G2S_HIP_TRY(hipMemcpy(ref_id, rows_.ref_id, m * 4, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(pos, rows_.pos, m * 4, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(end, rows_.end, m * 8, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(flag, rows_.flag, m * 4, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(h_own, rows_.h_own, m * 8, hipMemcpyDeviceToHost));
  G2S_HIP_TRY(hipMemcpy(h_mate, rows_.h_mate, m * 8, hipMemcpyDeviceToHost));
  return true;
}

bool BamRowsDevice::download_store(std::vector<uint8_t>* store, std::vector<uint64_t>* rec_off, std::string* why) const {
  store->assign((size_t)std::min<uint64_t>(stream_bytes_, store_ ? store_->capacity() : 0), 0);
  rec_off->assign((size_t)std::min<uint64_t>(rows_.n, cap_rows_), 0);
  G2S_HIP_TRY(hipSetDevice(device_));
  if (!store->empty()) G2S_HIP_TRY(hipMemcpy(store->data(), stream_buf_, store->size(), hipMemcpyDeviceToHost));
  if (!rec_off->empty()) G2S_HIP_TRY(hipMemcpy(rec_off->data(), rows_.rec_off, rec_off->size() * 8, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace g2s
