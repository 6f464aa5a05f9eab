// gap2seq_amd/csrc/bam_store.hip — see bam_store.h.  The store's kernels, per walk window on the reader's stream behind
// the row kernels (bam_rows.hip), before the window's inflate slot is written again:
//   lengths   k_store_len    one thread a record of this walk window: its stored size as a 64-bit count, 0 beyond the
//                            window's record count (read from the row kernels' control block on the device).  The record's
//                            layout is checked against the window's extent once more: the carried bytes in front, and the
//                            window's end.
//   offsets                  one exclusive 64-bit scan (rocPRIM) over capacity + 1 entries; entry `capacity` is the
//                            window's total
//   copy      k_store_write  a wave a record, the lanes over the record's stored bytes, 64 consecutive bytes a step, so
//                            that a wave's store is one run whatever the read's length (bam_text.hip: k_decode).  The two
//                            rewritten head fields are written by value.  rec_off[row_base + rank] = position + scan[rank].
//   position  k_store_next   one thread: the store position moves past the window
// Every store and every rec_off write is checked against its capacity first; a record that would not fit sets the
// overflow word and writes nothing.  The host waits for no window: it reads the position and the words once, in finish().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "bam_store.h"
#include "hip_host.h"

namespace {

using namespace g2s::bam_store;  // (kHead, stored_bytes, head_byte)

constexpr uint32_t kBlock = 256, kWave = 64;

// the store's state on the device: read and advanced by the kernels of one walk window after another, read by the host
// once, at the file's end
struct StorePos {
  unsigned long long at;       // where the next walk window's records begin in the store
  unsigned long long records;  // records met
  uint32_t over;               // a record had no room in the store (or its row no place in rec_off)
  uint32_t bad;                // a record outside its window, or a layout outside its block_size
};

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// (cap + 1 entries: every entry from the window's count on is 0, so that the scan's entry cap is the window's total)
__global__ void __launch_bounds__(kBlock) k_store_len(const uint8_t* __restrict__ win, int64_t front, int64_t end,
                                                      const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ n_rec,
                                                      const uint64_t* __restrict__ row_base, const uint32_t* __restrict__ anomaly,
                                                      uint32_t cap, uint64_t rows_cap, uint64_t* __restrict__ len, StorePos* pos) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r > cap) return;
  const uint32_t n = *anomaly ? 0u : (*n_rec < cap ? *n_rec : cap);  // (after an anomaly the rows are stale)
  uint64_t out = 0;
  if (r < n) {
    const uint64_t row = *row_base + r;
    bool ok = row < rows_cap;
    if (ok) {
      const int64_t o = (int64_t)rec_off[row];
      ok = o >= -front && o <= end && (int64_t)kHead <= end - o;
      if (ok) {
        const uint8_t* rec = win + o;
        const uint32_t bs = ld32(rec), l_name = rec[12], n_cigar = ld32(rec + 16) & 0xFFFFu;
        const int32_t l_seq = (int32_t)ld32(rec + 20);
        ok = l_seq >= 0 && l_name != 0 && 4 + (uint64_t)bs <= (uint64_t)(end - o) &&
             32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 <= bs;
        if (ok) out = stored_bytes(l_name, (uint64_t)l_seq);
      }
    }
    if (!ok) pos->bad = 1;
  }
  len[r] = out;
}

// off: the scan of k_store_len's counts; record r of the window goes to store[pos->at + off[r], pos->at + off[r + 1])
__global__ void __launch_bounds__(kBlock) k_store_write(const uint8_t* __restrict__ win, const uint32_t* __restrict__ n_rec,
                                                        const uint64_t* __restrict__ row_base, const uint32_t* __restrict__ anomaly,
                                                        uint32_t cap, const uint64_t* __restrict__ off, uint8_t* __restrict__ store,
                                                        uint64_t store_cap, uint64_t* rec_off, uint64_t rows_cap, StorePos* pos) {
  if (*anomaly) return;
  const uint32_t n = *n_rec < cap ? *n_rec : cap;  // (rows beyond the count have no bytes)
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t waves = gridDim.x * (kBlock / kWave);
  const uint64_t at = pos->at, base = *row_base;
  for (uint32_t r = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; r < n; r += waves) {
    const uint64_t a0 = off[r], a1 = off[r + 1], row = base + r;
    if (a1 == a0 || row >= rows_cap) continue;  // (a record k_store_len refused: the bad word is set)
    const uint64_t stored = a1 - a0;
    if (a1 > store_cap || at > store_cap - a1) {
      if (lane == 0) pos->over = 1;
      continue;
    }
    const uint8_t* rec = win + (int64_t)rec_off[row];  // (read by every lane before lane 0 replaces it below)
    const uint32_t l_name = rec[12], n_cigar = ld32(rec + 16) & 0xFFFFu;
    const uint8_t* seq = rec + kHead + l_name + 4 * (size_t)n_cigar;
    const uint64_t body = (uint64_t)kHead + l_name;  // head and name are one run of the source, the bases another
    uint8_t* dst = store + at + a0;
    for (uint64_t i = lane; i < stored; i += kWave)
      dst[i] = i < kHead ? head_byte((uint32_t)i, rec[i], stored) : i < body ? rec[i] : seq[i - body];
    if (lane == 0) rec_off[row] = at + a0;
  }
}

// one thread, behind k_store_write: the store position and the record count move past the window
__global__ void k_store_next(const uint64_t* __restrict__ off, uint32_t cap, const uint32_t* __restrict__ n_rec,
                             const uint32_t* __restrict__ anomaly, StorePos* pos) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || *anomaly) return;
  pos->at += off[cap];
  pos->records += *n_rec < cap ? *n_rec : cap;
}

}  // namespace

namespace g2s {

// the object's device allocations: freed by their destructors, the last declared first
struct BamStoreDevice::Buffers {
  DevMem store, work;
  uint64_t *len = nullptr, *off = nullptr;
  StorePos* pos = nullptr;
  Scratch tmp;  // (a piece of `work`)
};

BamStoreDevice* BamStoreDevice::create(int device, void* stream, uint64_t store_cap, uint64_t rows_cap, uint32_t ring_cap,
                                       std::string* why) {
  BamStoreDevice* S = new BamStoreDevice();
  Buffers& B = *(S->buf_ = new Buffers());
  S->device_ = device;
  S->stream_ = stream;
  S->store_cap_ = store_cap;
  S->rows_cap_ = rows_cap;
  S->ring_cap_ = ring_cap;
  auto make = [&]() -> bool {
    G2S_HIP_TRY(hipSetDevice(device));
    const size_t m = (size_t)ring_cap + 1, arr = (m * 8 + 255) & ~(size_t)255;
    size_t tb = 0;
    G2S_HIP_TRY(exclusive_scan_bytes<uint64_t>(m, &tb, (hipStream_t)stream));
    G2S_HIP_TRY(B.store.alloc((size_t)store_cap));
    G2S_HIP_TRY(B.work.alloc(2 * arr + 256 + tb));
    B.len = B.work.as<uint64_t>();
    B.off = (uint64_t*)(B.work.as<uint8_t>() + arr);
    B.pos = (StorePos*)(B.work.as<uint8_t>() + 2 * arr);
    B.tmp.p = B.work.as<uint8_t>() + 2 * arr + 256;
    B.tmp.bytes = tb;
    S->store_ = B.store.as<uint8_t>();
    G2S_HIP_TRY(hipMemsetAsync(B.pos, 0, sizeof(StorePos), (hipStream_t)stream));
    return true;
  };
  if (!make()) {
    (void)hipGetLastError();
    delete S;
    return nullptr;
  }
  return S;
}

BamStoreDevice::~BamStoreDevice() {
  if (device_ >= 0) (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
  delete buf_;
}

bool BamStoreDevice::window(const uint8_t* d_win, size_t front, size_t end, const uint32_t* n_rec, const uint64_t* row_base,
                            const uint32_t* anomaly, uint64_t* rec_off, std::string* why) {
  hipStream_t s = (hipStream_t)stream_;
  Buffers& B = *buf_;
  const size_t m = (size_t)ring_cap_ + 1;
  hipLaunchKernelGGL(k_store_len, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_win, (int64_t)front, (int64_t)end,
                     (const uint64_t*)rec_off, n_rec, row_base, anomaly, ring_cap_, rows_cap_, B.len, B.pos);
  G2S_HIP_TRY(hipGetLastError());
  G2S_HIP_TRY(exclusive_scan(B.tmp, B.len, B.off, m, s));
  const unsigned waves_wanted = (ring_cap_ + kWave - 1) / kWave;
  const unsigned groups = std::max(1u, std::min((waves_wanted + kBlock / kWave - 1) / (kBlock / kWave), 256u * 16u));
  hipLaunchKernelGGL(k_store_write, dim3(groups), dim3(kBlock), 0, s, d_win, n_rec, row_base, anomaly, ring_cap_,
                     (const uint64_t*)B.off, store_, store_cap_, rec_off, rows_cap_, B.pos);
  hipLaunchKernelGGL(k_store_next, dim3(1), dim3(1), 0, s, (const uint64_t*)B.off, ring_cap_, n_rec, anomaly, B.pos);
  G2S_HIP_TRY(hipGetLastError());
  return true;
}

bool BamStoreDevice::finish(uint64_t* used_bytes, uint64_t* records, bool* overflow, bool* bad, std::string* why) {
  StorePos pos{};
  G2S_HIP_TRY(hipSetDevice(device_));
  G2S_HIP_TRY(hipMemcpyAsync(&pos, buf_->pos, sizeof pos, hipMemcpyDeviceToHost, (hipStream_t)stream_));
  G2S_HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
  *used_bytes = pos.at;
  *records = pos.records;
  *overflow = pos.over != 0;
  *bad = pos.bad != 0;
  return true;
}

}  // namespace g2s
