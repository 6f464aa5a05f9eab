// gap2seq_amd/csrc/bam_reads.hip — see bam_reads.h.  A BAM file's part of the build's text: the host route, and the two
// kernels that make it from the inflated stream and the rows pass A's kernels leave in device memory.
// Every index is checked against its array's size before a write; a record that does not lie within the stream sets a
// flag that fails the device route (the caller then takes the host route).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bam.hpp"
#include "bam_decode.h"
#include "bam_reads.h"
#include "bam_rows.h"
#include "hip_host.h"
#include "readfilter_gaps.hpp"

namespace {

using namespace g2s::bam_decode;  // (kWave, kRecHead, ld32, kBases, emit)

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSkip = g2s::BAM_SECONDARY | g2s::BAM_SUPPLEMENTARY;

// what comes down between the scan and the text, in one copy
struct Totals {
  uint32_t bad;   // a record outside the stream, or a layout outside its block_size
  uint32_t over;  // a row's bytes had no room in the text
  unsigned long long kept;
};

// (n + 1 entries: entry n is 0, so that the scan's entry n is the total)
__global__ void __launch_bounds__(kBlock) k_bamreads_len(const uint8_t* __restrict__ stream, uint64_t stream_bytes,
                                                         const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ flag,
                                                         uint64_t n, uint64_t* __restrict__ len, Totals* tot) {
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  uint64_t out = 0;
  bool kept = false;
  if (r < n) {
    const uint64_t off = rec_off[r];
    bool ok = off <= stream_bytes && kRecHead <= stream_bytes - off;
    if (ok) {
      const uint8_t* rec = stream + off;
      const uint32_t bs = ld32(rec), l_name = rec[12], n_cigar = ld32(rec + 16) & 0xFFFFu;
      const int32_t l_seq = (int32_t)ld32(rec + 20);
      ok = l_seq >= 0 && l_name != 0 && 4 + (uint64_t)bs <= stream_bytes - off &&
           32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 <= bs;
      kept = ok && !(flag[r] & kSkip);
      if (kept) out = (uint64_t)l_seq + 1;
    }
    if (!ok) tot->bad = 1;
  }
  len[r] = out;
  const uint64_t mask = __ballot(kept);  // one addition a wave
  if (kept && (threadIdx.x % kWave) == (uint32_t)__builtin_ctzll(mask)) atomicAdd(&tot->kept, (unsigned long long)__popcll(mask));
}

// off: the scan of k_bamreads_len's counts; row r's bytes go to text[at + off[r], at + off[r + 1])
__global__ void __launch_bounds__(kBlock) k_bamreads_write(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ rec_off,
                                                           uint64_t n, const uint64_t* __restrict__ off, uint8_t* __restrict__ text,
                                                           uint64_t at, uint64_t cap, Totals* tot) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t chunks = (n + kWave - 1) / kWave;
  for (uint64_t c = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; c < chunks; c += waves) {
    const uint64_t mine = c * kWave + lane;
    const bool some = mine < n && off[mine + 1] != off[mine];
    uint64_t mask = __ballot(some);
    while (mask) {
      const uint64_t r = c * kWave + (uint64_t)__builtin_ctzll(mask);
      mask &= mask - 1;
      const uint64_t a0 = off[r], a1 = off[r + 1];
      if (a1 <= cap && at <= cap - a1) emit<kBases>(stream + rec_off[r], a1 - a0, text + at + a0, lane);
      else if (lane == 0) tot->over = 1;
    }
  }
}

}  // namespace

namespace g2s {

bool bam_reads_host(const ReadsInput& in, std::vector<std::string>* seqs, uint64_t* skipped, uint64_t* raw_bytes, std::string* err) {
  const std::string name = in.path.empty() ? "(memory)" : in.path;
  BamFile bam;
  std::string why;
  const bool opened = in.mem || in.path.empty() ? bam.open_mem(in.mem, in.mem_n, &why) : bam.open_path(in.path, &why);
  if (!opened) { *err = name + ": " + why; return false; }
  bam.reset_inflate_stats();
  const bool walked = bam.for_each([&](const BamRec& r) {
    if (r.flag & (BAM_SECONDARY | BAM_SUPPLEMENTARY)) {
      if (skipped) ++*skipped;
      return true;
    }
    seqs->emplace_back();
    append_bases(r, &seqs->back());
    return true;
  }, &why);
  if (!walked) { *err = name + ": " + why; return false; }
  if (raw_bytes) *raw_bytes += bam.inflate_stats().bytes_out;
  return true;
}

struct BamReadsDevice::Work {
  DevMem all;
  uint64_t *len = nullptr, *off = nullptr;
  Totals* tot = nullptr;
};

BamReadsDevice::BamReadsDevice() {}
BamReadsDevice::~BamReadsDevice() {
  work_.reset();
  rows_.reset();  // (its stream is the reader's)
  bam_.reset();
}

void* BamReadsDevice::stream() const { return rows_ ? rows_->stream() : nullptr; }

BamReadsDevice::Result BamReadsDevice::prepare(const ReadsInput& in, int device, size_t window, uint64_t resident_cap,
                                               int* reason, int* anomaly, std::string* why) {
  const std::string name = in.path.empty() ? "(memory)" : in.path;
  *reason = kBamReadsHip;
  *anomaly = kRowsOk;
  bam_.reset(new BamFile());
  std::string w;
  const bool opened = in.mem || in.path.empty() ? bam_->open_mem(in.mem, in.mem_n, &w) : bam_->open_path(in.path, &w);
  if (!opened) { *why = name + ": " + w; return kIoError; }
  bam_->set_window_bytes(window);
  bam_->set_inflate_device(device);
  int refused = kResidentKept;
  rows_.reset(bam_->rows_on_device(window, anomaly, &w, true, resident_cap, &refused));
  windows_ = bam_->rows_windows();
  if (!rows_) {
    *reason = *anomaly == kRowsHip ? kBamReadsHip : kBamReadsAnomaly;
    *why = "BAM rows: " + w;
    return kGaveUp;
  }
  if (refused != kResidentKept || !rows_->stream_buffer() || !rows_->rows().rec_off) {
    *reason = refused == kResidentNoMemory ? kBamReadsHip : kBamReadsOverCap;
    *why = refused == kResidentNoMemory ? "no memory for the inflated BAM stream" : "the inflated BAM stream and its rows are over the cap";
    return kGaveUp;
  }
  stream_bytes_ = rows_->stream_bytes();
  rows_n_ = rows_->rows().n;
  resident_bytes_ = stream_bytes_ + 64 + (stream_bytes_ / 36 + 2) * 52;  // (bam_rows.hip: BamRowsDevice::create)
  bool bad = false;
  if (!count(&bad, &w)) {
    *why = "BAM text: " + w;
    return kGaveUp;
  }
  if (bad) {
    *reason = kBamReadsAnomaly;
    *anomaly = kRowsDeadLink;
    *why = "BAM text: a record outside the resident stream";
    return kGaveUp;
  }
  *reason = kBamReadsKernels;
  return kOk;
}

// the lengths, their scan, the totals down
bool BamReadsDevice::count(bool* bad, std::string* why) {
  const uint64_t n = rows_n_;
  const DeviceRows& R = rows_->rows();
  hipStream_t s = (hipStream_t)rows_->stream();
  G2S_HIP_TRY(hipSetDevice(rows_->device()));
  const size_t m = (size_t)n + 1;
  size_t tb = 0;
  G2S_HIP_TRY(exclusive_scan_bytes<uint64_t>(m, &tb, s));
  const size_t arr = (m * 8 + 255) & ~(size_t)255;
  work_.reset(new Work());
  G2S_HIP_TRY(work_->all.alloc(2 * arr + 256 + tb));
  work_->len = work_->all.as<uint64_t>();
  work_->off = (uint64_t*)(work_->all.as<uint8_t>() + arr);
  work_->tot = (Totals*)(work_->all.as<uint8_t>() + 2 * arr);
  Scratch tmp;  // (a piece of the same allocation)
  tmp.p = work_->all.as<uint8_t>() + 2 * arr + 256;
  tmp.bytes = tb;
  G2S_HIP_TRY(hipMemsetAsync(work_->tot, 0, sizeof(Totals), s));
  hipLaunchKernelGGL(k_bamreads_len, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     (const uint8_t*)rows_->stream_buffer(), stream_bytes_, (const uint64_t*)R.rec_off, (const uint32_t*)R.flag, n,
                     work_->len, work_->tot);
  G2S_HIP_TRY(hipGetLastError());
  G2S_HIP_TRY(exclusive_scan(tmp, work_->len, work_->off, m, s));
  Totals tot{};
  uint64_t total = 0;
  G2S_HIP_TRY(hipMemcpyAsync(&tot, work_->tot, sizeof tot, hipMemcpyDeviceToHost, s));
  G2S_HIP_TRY(hipMemcpyAsync(&total, work_->off + n, 8, hipMemcpyDeviceToHost, s));
  G2S_HIP_TRY(hipStreamSynchronize(s));
  kept_ = tot.kept;
  text_bytes_ = tot.bad ? 0 : total;
  *bad = tot.bad != 0;
  return true;
}

bool BamReadsDevice::write(uint8_t* d_text, uint64_t at, uint64_t cap, std::string* why) {
  const uint64_t n = rows_n_;
  if (!n || !text_bytes_) return true;
  hipStream_t s = (hipStream_t)rows_->stream();
  G2S_HIP_TRY(hipSetDevice(rows_->device()));
  const unsigned waves_wanted = (unsigned)((n + kWave - 1) / kWave);
  const unsigned groups = std::max(1u, std::min((waves_wanted + kBlock / kWave - 1) / (kBlock / kWave), 256u * 16u));
  hipLaunchKernelGGL(k_bamreads_write, dim3(groups), dim3(kBlock), 0, s, (const uint8_t*)rows_->stream_buffer(),
                     (const uint64_t*)rows_->rows().rec_off, n, (const uint64_t*)work_->off, d_text, at, cap, work_->tot);
  G2S_HIP_TRY(hipGetLastError());
  Totals tot{};
  G2S_HIP_TRY(hipMemcpyAsync(&tot, work_->tot, sizeof tot, hipMemcpyDeviceToHost, s));
  G2S_HIP_TRY(hipStreamSynchronize(s));
  if (tot.over) {
    if (why) *why = "the BAM text outgrew its buffer";
    return false;
  }
  return true;
}

}  // namespace g2s
