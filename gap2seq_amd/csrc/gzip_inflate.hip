// gap2seq_amd/csrc/gzip_inflate.hip — see gzip_inflate.h.  The kernels that run gzip_chunks.h on the GPU, the two
// backends, and the route over a file's members and windows.
//
// Per window, on one stream, no workgroup waits for another inside a launch:
//   k_gz_find     one wave a chunk: 64 bit offsets side by side through prefilter(), the lanes that survive verified one
//                 after another by the wave-uniform accept_start(); the first accepted offset of the chunk
//   k_gz_decode   one wave a chunk that has a start, claimed by a ticket.  The decoder is wave-uniform, as in
//                 g2s_bgzf_inflate.  History is a ring of 32 768 16-bit symbols in LDS (64 KiB) beside the tables
//                 (4.1 KiB): 68.3 KiB a workgroup, two a CU.  Every symbol is written to the ring and to the chunk's slot
//                 in device memory at once — the ring serves the back-references, the slot is what leaves; up to 64
//                 pending literals go by one instruction, a match is copied by the lanes together
//   k_gz_chain    one workgroup: the resolved 32 768-byte window behind every chunk, in chunk order
//   k_gz_resolve  every symbol to its byte, contiguously at the chunk's offset (the host's prefix sum of the chunks'
//                 output counts, which it has read with their states anyway)
//   k_gz_crc      the CRC-32 of spans of 256 KiB, a thread a KiB, combined within the workgroup; the host combines the
//                 spans (inflate_core.h: crc_shift64)
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gzip_chunks.h"
#include "gzip_inflate.h"
#include "hip_host.h"
#include "readfilter_gaps.hpp"

namespace {

namespace inf = g2s::inflate;
namespace gz = g2s::gzchunks;
constexpr uint32_t kWave = 64;
constexpr uint32_t kCrcThreads = 256, kCrcSlice = 1024, kCrcSpan = kCrcThreads * kCrcSlice;
constexpr uint32_t kChainThreads = 1024, kResolveThreads = 256, kResolveBlocks = 64;

struct GzJob {  // (GzipBackend::Job)
  uint64_t start, stop, slot_off;
  uint32_t cap, first;
  uint32_t status, out_n;
  uint64_t end_bit;
};
struct GzPlace {  // (GzipBackend::Place)
  uint64_t slot_off, out_off;
  uint32_t out_n, valid;
};

// the wave's sink: the ring in LDS and the slot in device memory
struct RingSink {
  uint16_t* ring;  // kWindow symbols, position p at ring[p mod kWindow]
  uint16_t* slot;
  uint32_t lane;
  uint32_t lit_at, nlit, mine;
  __device__ __forceinline__ void order() { __builtin_amdgcn_wave_barrier(); }
  __device__ __forceinline__ void store(uint32_t at, uint16_t v) {
    ring[at & (gz::kWindow - 1u)] = v;
    slot[at] = v;
  }
  __device__ __forceinline__ void flush() {
    if (lane < nlit) store(lit_at + lane, (uint16_t)mine);
    nlit = 0;
    order();
  }
  __device__ __forceinline__ void put(uint32_t at, uint16_t c) {
    if (nlit == 0) lit_at = at;
    if (lane == nlit) mine = c;
    if (++nlit == kWave) flush();
  }
  // Lane i takes symbol i, i + 64, ... of the match.  Every source lies in front of the match, so the overlapping case
  // needs no order among the lanes; the ring cell a lane reads is one the match writes only when distance > 32 768 - 258,
  // and then by the same lane or a lane further on, which stores after every lane of its round has read.
  __device__ __forceinline__ void match(uint32_t at, uint32_t dist, uint32_t len) {
    if (nlit) flush();
    for (uint32_t i = lane; i < len; i += kWave) {
      const int64_t s = (int64_t)at - (int64_t)dist + (int64_t)(dist >= len ? i : i % dist);
      const uint16_t v = s < 0 ? gz::marker_of(s) : ring[(uint32_t)s & (gz::kWindow - 1u)];
      order();
      store(at + i, v);
    }
    order();
  }
  __device__ __forceinline__ void copy_in(uint32_t at, const uint8_t* from, uint32_t len) {
    if (nlit) flush();
    for (uint32_t i = lane; i < len; i += kWave) store(at + i, from[i]);
    order();
  }
  __device__ __forceinline__ void finish() {
    if (nlit) flush();
  }
};

}  // namespace

__global__ void __launch_bounds__(64) k_gz_find(const uint8_t* __restrict__ comp, uint32_t n, uint32_t chunk, uint32_t nchunks,
                                                uint64_t* __restrict__ starts) {
  __shared__ inf::Tables tables;
  const uint32_t c = blockIdx.x + 1u, lane = threadIdx.x;
  if (c >= nchunks) return;
  const uint64_t lo = (uint64_t)c * chunk * 8u;
  const uint64_t end = (uint64_t)(c + 1u) * chunk < n ? (uint64_t)(c + 1u) * chunk : n;
  const uint64_t hi = end * 8u;
  uint64_t found = gz::kNoBit;
  for (uint64_t base = lo; base < hi && found == gz::kNoBit; base += kWave) {
    const uint64_t bit = base + lane;
    const bool ok = bit < hi && gz::prefilter(comp, n, bit);
    uint64_t m = __ballot(ok);
    while (m) {
      const uint32_t j = (uint32_t)__ffsll((long long)m) - 1u;
      m &= m - 1u;
      if (gz::accept_start(comp, n, base + j, &tables)) { found = base + j; break; }
    }
  }
  if (lane == 0) starts[c] = found;
}

__global__ void __launch_bounds__(64) k_gz_decode(const uint8_t* __restrict__ comp, uint32_t n, GzJob* __restrict__ jobs,
                                                  uint32_t njobs, uint16_t* __restrict__ slots, uint32_t* __restrict__ ticket) {
  __shared__ uint16_t ring[gz::kWindow];
  __shared__ inf::Tables tables;
  const uint32_t lane = threadIdx.x;
  for (;;) {
    uint32_t j = 0;
    if (lane == 0) j = atomicAdd(ticket, 1u);
    j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
    if (j >= njobs) break;
    const GzJob job = jobs[j];
    RingSink sink{ring, slots + job.slot_off, lane, 0, 0, 0};
    const gz::ChunkEnd e = gz::decode_chunk(comp, n, job.start, job.stop, job.first != 0, job.cap, &tables, sink);
    if (lane == 0) {
      jobs[j].status = e.status;
      jobs[j].out_n = e.out_n;
      jobs[j].end_bit = e.end_bit;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// hist: m + 1 windows of kWindow bytes, window 0 the one in front of the first chunk
__global__ void __launch_bounds__(kChainThreads) k_gz_chain(const GzPlace* __restrict__ places, uint32_t m,
                                                            const uint16_t* __restrict__ slots, uint8_t* hist) {
  for (uint32_t c = 0; c < m; c++) {
    const uint8_t* prev = hist + (size_t)c * gz::kWindow;
    uint8_t* next = hist + (size_t)(c + 1u) * gz::kWindow;
    const uint16_t* slot = slots + places[c].slot_off;
    const uint32_t out_n = places[c].out_n;
    for (uint32_t j = threadIdx.x; j < gz::kWindow; j += kChainThreads) next[j] = gz::chain_byte(prev, slot, out_n, j);
    __syncthreads();
  }
}

// blockIdx.y: the chunk
__global__ void __launch_bounds__(kResolveThreads) k_gz_resolve(const GzPlace* __restrict__ places,
                                                                const uint16_t* __restrict__ slots,
                                                                const uint8_t* __restrict__ hist, uint8_t* __restrict__ out,
                                                                uint32_t* __restrict__ bad) {
  const GzPlace p = places[blockIdx.y];
  const uint16_t* slot = slots + p.slot_off;
  const uint8_t* h = hist + (size_t)blockIdx.y * gz::kWindow;
  uint8_t* dst = out + p.out_off;
  bool wrong = false;
  for (uint32_t i = blockIdx.x * kResolveThreads + threadIdx.x; i < p.out_n; i += gridDim.x * kResolveThreads) {
    const uint16_t s = slot[i];
    wrong |= !gz::sym_ok(s, p.valid);
    dst[i] = gz::resolve_sym(s, h);
  }
  if (wrong) atomicOr(bad, 1u);
}

// span_crc[b]: the finished CRC-32 of bytes [b * kCrcSpan, (b + 1) * kCrcSpan) clipped to n
__global__ void __launch_bounds__(kCrcThreads) k_gz_crc(const uint8_t* __restrict__ bytes, uint64_t n,
                                                        uint32_t* __restrict__ span_crc) {
  __shared__ uint32_t table[256];
  __shared__ uint32_t part[kCrcThreads / kWave];
  for (uint32_t i = threadIdx.x; i < 256u; i += kCrcThreads) table[i] = inf::crc_table_entry(i);
  __syncthreads();
  const uint64_t span_lo = (uint64_t)blockIdx.x * kCrcSpan, span_hi = span_lo + kCrcSpan < n ? span_lo + kCrcSpan : n;
  const uint64_t lo0 = span_lo + (uint64_t)threadIdx.x * kCrcSlice, lo = lo0 < span_hi ? lo0 : span_hi;
  const uint64_t hi = lo + kCrcSlice < span_hi ? lo + kCrcSlice : span_hi;
  uint32_t c = 0;
  if (hi > lo) {
    c = 0xFFFFFFFFu;
    for (uint64_t o = lo; o < hi; o++) c = inf::crc_byte(table, c, bytes[o]);
    c = inf::crc_shift(~c, (uint32_t)(span_hi - hi));
  }
  for (int off = 32; off; off >>= 1) c ^= (uint32_t)__shfl_xor((int)c, off, 64);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t x = 0;
    for (uint32_t w = 0; w < kCrcThreads / kWave; w++) x ^= part[w];
    span_crc[blockIdx.x] = x;
  }
}

namespace g2s {

namespace {

std::atomic<int> g_device_gzip{-1};

uint64_t slot_symbols(const GzipParams& P, uint32_t chunks) { return (uint64_t)chunks * P.chunk * P.ratio; }

}  // namespace

int set_device_gzip(int mode) { return g_device_gzip.exchange(mode < 0 ? -1 : mode > 0 ? 1 : 0); }
bool device_gzip_asked() {
  const int m = g_device_gzip.load();
  if (m >= 0) return m > 0;
  const char* s = getenv("G2S_DEVICE_GZIP");
  return s && strcmp(s, "1") == 0;
}
GzipParams gzip_params_from_env() {
  GzipParams P;
  auto num = [](const char* name) -> uint64_t {
    const char* s = getenv(name);
    return s && *s ? strtoull(s, nullptr, 10) : 0;
  };
  if (const uint64_t v = num("G2S_GZIP_CHUNK_BYTES")) P.chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(v, 1024), 64u << 20);
  if (const uint64_t v = num("G2S_GZIP_WINDOW_CHUNKS")) P.window_chunks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(v, 2), 65535);
  if (const uint64_t v = num("G2S_GZIP_SLOT_RATIO")) P.ratio = (uint32_t)std::min<uint64_t>(v, 1024);
  return P;
}

size_t gzip_header_bytes(const uint8_t* p, size_t left) {
  if (left < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xE0)) return 0;
  const uint32_t flg = p[3];
  size_t at = 10;
  if (flg & 4u) {
    if (at + 2 > left) return 0;
    at += 2 + ((size_t)p[at] | (size_t)p[at + 1] << 8);
    if (at > left) return 0;
  }
  for (uint32_t bit : {8u, 16u}) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (at < left && p[at]) at++;
    if (at >= left) return 0;
    at++;
  }
  if (flg & 2u) {
    if (at + 2 > left) return 0;
    const uint32_t want = (uint32_t)p[at] | (uint32_t)p[at + 1] << 8;
    if ((crc32(0L, p, (uInt)at) & 0xFFFFu) != want) return 0;
    at += 2;
  }
  return at;
}

// ---- a window's four steps, the same for both backends
GzipWindow GzipBackend::window(const uint8_t* comp, size_t n, uint32_t start_bit, bool first, uint32_t valid, bool to_end,
                               const GzipParams& P, uint32_t nchunks, uint32_t front) {
  GzipWindow r;
  auto refuse = [&](int outcome) { r.outcome = outcome; return r; };
  if (!load(comp, n, first)) return refuse(kGzHip);
  std::vector<uint64_t> starts(nchunks, gz::kNoBit);
  starts[0] = start_bit;
  if (nchunks > 1 && !find(P.chunk, nchunks, starts.data())) return refuse(kGzHip);
  std::vector<uint32_t> at;  // the chunks that have a start
  for (uint32_t c = 0; c < nchunks; c++)
    if (starts[c] != gz::kNoBit) at.push_back(c);
  r.found = (uint32_t)at.size() - 1u;
  if (!to_end && at.size() < 2) return refuse(kGzTooFewStarts);
  // a window that does not reach the file's end stops at its last start: the next window begins there
  const uint32_t njobs = (uint32_t)(to_end ? at.size() : at.size() - 1);
  r.covered = to_end ? nchunks : at[njobs];
  std::vector<Job> jobs(njobs);
  for (uint32_t i = 0; i < njobs; i++) {
    const uint32_t c = at[i], behind = i + 1 < at.size() ? at[i + 1] : nchunks;
    Job& j = jobs[i];
    j.start = starts[c];
    j.stop = i + 1 < at.size() ? starts[at[i + 1]] : gz::kNoBit;
    j.slot_off = slot_symbols(P, c);
    // (an absorbing chunk writes on through the slots of the chunks it absorbed)
    j.cap = (uint32_t)std::min<uint64_t>(slot_symbols(P, behind - c), 0x7FFFFFFFu);
    j.first = first && i == 0 ? 1u : 0u;
    j.status = gz::kEndCorrupt;
    j.out_n = 0;
    j.end_bit = 0;
  }
  if (!decode(jobs.data(), njobs)) return refuse(kGzHip);
  std::vector<Place> places;
  uint64_t produced = valid;
  for (uint32_t i = 0; i < njobs && !r.final; i++) {
    const Job& j = jobs[i];
    switch (j.status) {
      case gz::kEndOk: break;
      case gz::kEndFinal:  // (what the chunks behind it decoded is another member's, or nothing: forgotten)
        r.final = true;
        r.end_byte = (j.end_bit + 7u) / 8u;
        r.covered = i + 1 < at.size() ? at[i + 1] : nchunks;
        break;
      case gz::kEndMismatch: return refuse(kGzMismatch);
      case gz::kEndSlotFull: return refuse(kGzSlotFull);
      default: return refuse(kGzCorrupt);
    }
    places.push_back(Place{j.slot_off, r.out_n, j.out_n, (uint32_t)std::min<uint64_t>(produced, gz::kWindow)});
    r.out_n += j.out_n;
    produced += j.out_n;
  }
  if (!r.final && to_end) return refuse(kGzCorrupt);  // (never: without a stop a chunk ends final or corrupt)
  r.jobs = (uint32_t)places.size();
  if (!r.final) r.next_bit = starts[at[njobs]];
  bool bad = false;
  if (!finish(places.data(), r.jobs, r.out_n, front, &r.crc, &bad)) return refuse(kGzHip);
  if (bad) return refuse(kGzCorrupt);
  return r;
}

namespace {

// ---- gzip_chunks.h compiled for the host, chunk by chunk
class HostBackend : public GzipBackend {
 public:
  explicit HostBackend(const GzipParams& P) : P_(P) {}
  const uint8_t* out() const override { return out_.data(); }

 protected:
  bool load(const uint8_t* comp, size_t n, bool first) override {
    comp_ = comp;
    n_ = (uint32_t)n;
    if (first) hist_.assign(gz::kWindow, 0);
    return true;
  }
  bool find(uint32_t chunk, uint32_t nchunks, uint64_t* starts) override {
    for (uint32_t c = 1; c < nchunks; c++) {
      const uint64_t lo = (uint64_t)c * chunk * 8u, hi = std::min<uint64_t>((uint64_t)(c + 1) * chunk, n_) * 8u;
      starts[c] = gz::find_start(comp_, n_, lo, hi, &T_);
    }
    return true;
  }
  bool decode(Job* jobs, uint32_t njobs) override {
    for (uint32_t i = 0; i < njobs; i++) {
      Job& j = jobs[i];
      if (slots_.size() < j.slot_off + j.cap) slots_.resize(j.slot_off + j.cap);
      gz::HostSymSink sink{slots_.data() + j.slot_off};
      const gz::ChunkEnd e = gz::decode_chunk(comp_, n_, j.start, j.stop, j.first != 0, j.cap, &T_, sink);
      j.status = e.status;
      j.out_n = e.out_n;
      j.end_bit = e.end_bit;
    }
    return true;
  }
  bool finish(const Place* places, uint32_t m, uint64_t out_n, uint32_t front, uint32_t* crc, bool* bad) override {
    out_.resize(front + out_n + 1);
    std::vector<uint8_t> next(gz::kWindow);
    for (uint32_t c = 0; c < m; c++) {
      const Place& p = places[c];
      const uint16_t* slot = slots_.data() + p.slot_off;
      for (uint32_t i = 0; i < p.out_n; i++) {
        if (!gz::sym_ok(slot[i], p.valid)) *bad = true;
        out_[front + p.out_off + i] = gz::resolve_sym(slot[i], hist_.data());
      }
      for (uint32_t j = 0; j < gz::kWindow; j++) next[j] = gz::chain_byte(hist_.data(), slot, p.out_n, j);
      hist_.swap(next);
    }
    // the CRC as the device takes it: slices, spans, combination
    uint32_t table[256];
    for (uint32_t i = 0; i < 256u; i++) table[i] = inf::crc_table_entry(i);
    uint32_t x = 0;
    for (uint64_t lo = 0; lo < out_n; lo += kCrcSlice) {
      const uint64_t hi = std::min<uint64_t>(lo + kCrcSlice, out_n);
      uint32_t c = 0xFFFFFFFFu;
      for (uint64_t o = lo; o < hi; o++) c = inf::crc_byte(table, c, out_[front + o]);
      x ^= inf::crc_shift64(~c, out_n - hi);
    }
    *crc = x;
    return true;
  }

 private:
  GzipParams P_;
  const uint8_t* comp_ = nullptr;
  uint32_t n_ = 0;
  inf::Tables T_;
  std::vector<uint16_t> slots_;
  std::vector<uint8_t> hist_, out_;
};

// ---- the kernels
class DeviceBackend : public GzipBackend {
 public:
  DeviceBackend(int device, hipStream_t st, const GzipParams& P) : device_(device), st_(st), P_(P) {}
  const uint8_t* out() const override { return d_out_.as<uint8_t>(); }
  uint64_t device_bytes() const override { return gzip_device_bytes(P_); }

  bool make(std::string* why) {
    const uint32_t W = P_.window_chunks;
    G2S_HIP_TRY(hipSetDevice(device_));
    G2S_HIP_TRY(d_comp_.alloc(comp_bytes(P_)));
    G2S_HIP_TRY(d_slots_.alloc(slot_symbols(P_, W) * 2u));
    G2S_HIP_TRY(d_out_.alloc(out_bytes(P_)));
    G2S_HIP_TRY(d_hist_.alloc(hist_bytes(P_)));
    G2S_HIP_TRY(d_small_.alloc(small_bytes(P_)));
    G2S_HIP_TRY(h_small_.alloc(small_bytes(P_)));
    return true;
  }
  static uint64_t comp_bytes(const GzipParams& P) { return (uint64_t)P.window_chunks * P.chunk + 16u; }
  static uint64_t out_bytes(const GzipParams& P) { return slot_symbols(P, P.window_chunks) + 32u; }
  static uint64_t hist_bytes(const GzipParams& P) { return ((uint64_t)P.window_chunks + 1u) * gz::kWindow; }
  static uint64_t spans(const GzipParams& P) { return slot_symbols(P, P.window_chunks) / kCrcSpan + 1u; }
  // jobs | places | starts | span CRCs | ticket, bad
  static uint64_t small_bytes(const GzipParams& P) {
    return (uint64_t)P.window_chunks * (sizeof(GzJob) + sizeof(GzPlace) + 8u) + spans(P) * 4u + 16u;
  }

 protected:
  uint8_t* small(void* base, uint64_t off) const { return (uint8_t*)base + off; }
  uint64_t off_places() const { return (uint64_t)P_.window_chunks * sizeof(GzJob); }
  uint64_t off_starts() const { return off_places() + (uint64_t)P_.window_chunks * sizeof(GzPlace); }
  uint64_t off_crc() const { return off_starts() + (uint64_t)P_.window_chunks * 8u; }
  uint64_t off_flags() const { return off_crc() + spans(P_) * 4u; }

  bool load(const uint8_t* comp, size_t n, bool first) override {
    std::string* why = &this->why;
    if (n + 16u > comp_bytes(P_) || n >= 0xFFFFFFF0u) { *why = "a window larger than its buffer"; return false; }
    n_ = (uint32_t)n;
    G2S_HIP_TRY(hipSetDevice(device_));
    G2S_HIP_TRY(hipMemcpyAsync(d_comp_.p, comp, n, hipMemcpyHostToDevice, st_));
    if (first) G2S_HIP_TRY(hipMemsetAsync(d_hist_.p, 0, gz::kWindow, st_));
    return true;
  }
  bool find(uint32_t chunk, uint32_t nchunks, uint64_t* starts) override {
    std::string* why = &this->why;
    uint64_t* d_starts = (uint64_t*)small(d_small_.p, off_starts());
    hipLaunchKernelGGL(k_gz_find, dim3(nchunks - 1u), dim3(kWave), 0, st_, d_comp_.as<uint8_t>(), n_, chunk, nchunks, d_starts);
    G2S_HIP_TRY(hipGetLastError());
    uint64_t* h_starts = (uint64_t*)small(h_small_.p, off_starts());
    G2S_HIP_TRY(hipMemcpyAsync(h_starts + 1, d_starts + 1, (size_t)(nchunks - 1u) * 8u, hipMemcpyDeviceToHost, st_));
    G2S_HIP_TRY(hipStreamSynchronize(st_));
    memcpy(starts + 1, h_starts + 1, (size_t)(nchunks - 1u) * 8u);
    return true;
  }
  bool decode(Job* jobs, uint32_t njobs) override {
    static_assert(sizeof(Job) == sizeof(GzJob) && sizeof(Place) == sizeof(GzPlace), "the kernels' layouts");
    std::string* why = &this->why;
    if (!njobs) return true;
    // every slot inside the allocation
    for (uint32_t i = 0; i < njobs; i++)
      if (jobs[i].slot_off + jobs[i].cap > slot_symbols(P_, P_.window_chunks)) { *why = "a slot beyond the window's"; return false; }
    GzJob* d_jobs = (GzJob*)d_small_.p;
    uint32_t* d_flags = (uint32_t*)small(d_small_.p, off_flags());
    memcpy(h_small_.p, jobs, (size_t)njobs * sizeof(GzJob));
    G2S_HIP_TRY(hipMemcpyAsync(d_jobs, h_small_.p, (size_t)njobs * sizeof(GzJob), hipMemcpyHostToDevice, st_));
    G2S_HIP_TRY(hipMemsetAsync(d_flags, 0, 16, st_));
    hipLaunchKernelGGL(k_gz_decode, dim3(std::min<uint32_t>(njobs, 512u)), dim3(kWave), 0, st_, d_comp_.as<uint8_t>(), n_, d_jobs,
                       njobs, d_slots_.as<uint16_t>(), d_flags);
    G2S_HIP_TRY(hipGetLastError());
    G2S_HIP_TRY(hipMemcpyAsync(h_small_.p, d_jobs, (size_t)njobs * sizeof(GzJob), hipMemcpyDeviceToHost, st_));
    G2S_HIP_TRY(hipStreamSynchronize(st_));
    memcpy(jobs, h_small_.p, (size_t)njobs * sizeof(GzJob));
    return true;
  }
  bool finish(const Place* places, uint32_t m, uint64_t out_n, uint32_t front, uint32_t* crc, bool* bad) override {
    std::string* why = &this->why;
    *crc = 0;
    *bad = false;
    if (front + out_n + 16u > out_bytes(P_)) { *why = "a window's bytes beyond their buffer"; return false; }
    if (m) {
      GzPlace* d_places = (GzPlace*)small(d_small_.p, off_places());
      uint32_t* d_flags = (uint32_t*)small(d_small_.p, off_flags());
      memcpy(small(h_small_.p, off_places()), places, (size_t)m * sizeof(GzPlace));
      G2S_HIP_TRY(hipMemcpyAsync(d_places, small(h_small_.p, off_places()), (size_t)m * sizeof(GzPlace), hipMemcpyHostToDevice, st_));
      hipLaunchKernelGGL(k_gz_chain, dim3(1), dim3(kChainThreads), 0, st_, (const GzPlace*)d_places, m,
                         (const uint16_t*)d_slots_.p, d_hist_.as<uint8_t>());
      G2S_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_gz_resolve, dim3(kResolveBlocks, m), dim3(kResolveThreads), 0, st_, (const GzPlace*)d_places,
                         (const uint16_t*)d_slots_.p, (const uint8_t*)d_hist_.p, d_out_.as<uint8_t>() + front, d_flags + 1);
      G2S_HIP_TRY(hipGetLastError());
      // the window behind the last chunk is the one in front of the next window's first
      G2S_HIP_TRY(hipMemcpyAsync(d_hist_.p, d_hist_.as<uint8_t>() + (size_t)m * gz::kWindow, gz::kWindow, hipMemcpyDeviceToDevice, st_));
    }
    const uint32_t nspans = (uint32_t)((out_n + kCrcSpan - 1u) / kCrcSpan);
    uint32_t* h_crc = (uint32_t*)small(h_small_.p, off_crc());
    if (nspans) {
      uint32_t* d_crc = (uint32_t*)small(d_small_.p, off_crc());
      hipLaunchKernelGGL(k_gz_crc, dim3(nspans), dim3(kCrcThreads), 0, st_, (const uint8_t*)d_out_.as<uint8_t>() + front, out_n, d_crc);
      G2S_HIP_TRY(hipGetLastError());
      // (the span CRCs and, right behind them, the flags)
      G2S_HIP_TRY(hipMemcpyAsync(h_crc, d_crc, (size_t)spans(P_) * 4u + 16u, hipMemcpyDeviceToHost, st_));
    } else {
      G2S_HIP_TRY(hipMemcpyAsync(small(h_small_.p, off_flags()), small(d_small_.p, off_flags()), 16, hipMemcpyDeviceToHost, st_));
    }
    G2S_HIP_TRY(hipStreamSynchronize(st_));
    uint32_t x = 0;
    for (uint32_t b = 0; b < nspans; b++) {
      const uint64_t hi = std::min<uint64_t>((uint64_t)(b + 1u) * kCrcSpan, out_n);
      x ^= inf::crc_shift64(h_crc[b], out_n - hi);
    }
    *crc = x;
    *bad = m && ((const uint32_t*)small(h_small_.p, off_flags()))[1] != 0;
    return true;
  }

 private:
  int device_;
  hipStream_t st_;
  GzipParams P_;
  uint32_t n_ = 0;
  DevMem d_comp_, d_slots_, d_out_, d_hist_, d_small_;
  PinMem h_small_;
};

}  // namespace

uint64_t gzip_device_bytes(const GzipParams& P) {
  return DeviceBackend::comp_bytes(P) + slot_symbols(P, P.window_chunks) * 2u + DeviceBackend::out_bytes(P) +
         DeviceBackend::hist_bytes(P) + DeviceBackend::small_bytes(P);
}

std::unique_ptr<GzipBackend> make_gzip_device_backend(int device, void* stream, const GzipParams& P, std::string* why) {
  if (!filter_device_usable(device)) {
    if (why) *why = "no usable gfx950 device " + std::to_string(device);
    return nullptr;
  }
  std::unique_ptr<DeviceBackend> B(new DeviceBackend(device, (hipStream_t)stream, P));
  if (!B->make(why)) return nullptr;
  return B;
}
std::unique_ptr<GzipBackend> make_gzip_host_backend(const GzipParams& P) { return std::unique_ptr<GzipBackend>(new HostBackend(P)); }

int gzip_route(const uint8_t* file, size_t n, const GzipParams& P, GzipBackend& backend, GzipStats* stats,
               const std::function<uint32_t()>& front, const std::function<bool(const uint8_t*, uint64_t, bool)>& deliver) {
  stats->files++;
  auto give_back = [&](int outcome) { stats->outcome = outcome; return outcome; };
  size_t pos = 0;
  uint64_t found = 0, covered = 0;
  for (;;) {  // members
    const size_t hdr = gzip_header_bytes(file + pos, n - pos);
    if (!hdr) return give_back(kGzHeader);
    size_t base = pos + hdr;
    uint32_t start_bit = 0, crc = 0;
    uint64_t isize = 0;
    bool first = true, file_done = false;
    for (;;) {  // windows
      const size_t avail = n - base;
      if (!avail) return give_back(kGzTrailer);
      const uint32_t nchunks = (uint32_t)std::min<uint64_t>(P.window_chunks, (avail + P.chunk - 1) / P.chunk);
      const size_t take = (size_t)std::min<uint64_t>(avail, (uint64_t)nchunks * P.chunk);
      const bool to_end = take == avail;
      const uint32_t fr = front();
      const GzipWindow w = backend.window(file + base, take, start_bit, first, (uint32_t)std::min<uint64_t>(isize, gz::kWindow),
                                          to_end, P, nchunks, fr);
      stats->windows++;
      if (w.outcome != kGzDone) return give_back(w.outcome);
      stats->chunks += w.covered;
      stats->starts_found += w.found;
      stats->absorbed += w.covered - w.jobs;
      found += w.found;
      covered += w.covered;
      if (P.quarter_rule && found * 4u < covered) return give_back(kGzTooFewStarts);
      crc = inf::crc_shift64(crc, w.out_n) ^ w.crc;
      isize += w.out_n;
      bool last = false;
      if (w.final) {
        const size_t end = base + (size_t)w.end_byte;
        if (end + 8 > n) return give_back(kGzTrailer);
        const uint8_t* t = file + end;
        const uint32_t want_crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t want_n = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (want_crc != crc || want_n != (uint32_t)isize) return give_back(kGzTrailer);
        stats->members++;
        pos = end + 8;
        last = pos == n;
        if (!last && !gzip_header_bytes(file + pos, n - pos)) return give_back(kGzHeader);
        file_done = last;
      } else {
        base += (size_t)(w.next_bit >> 3);
        start_bit = (uint32_t)w.next_bit & 7u;
        first = false;
      }
      if (!deliver(backend.out() + fr, w.out_n, last)) return give_back(kGzHip);
      if (w.final) break;
    }
    if (file_done) break;
  }
  return give_back(kGzDone);
}

}  // namespace g2s
