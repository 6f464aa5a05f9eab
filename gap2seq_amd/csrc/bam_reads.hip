// gap2seq_amd/csrc/bam_reads.hip — see bam_reads.h.  A BAM file's part of the build's text: the host route, and the two
// kernels that make it from the inflated stream and the rows pass A's kernels leave in device memory — resident, from
// the whole stream and whole-file rows, or streaming, from one walk window and its ring of compact rows at a time.
// Every index is checked against its array's size before a write; a record that does not lie within the stream (within
// its window) sets a flag that fails the device route (the caller then takes the host route).
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

// the streaming form's state on the device, beside the loader's carry: read and advanced by the kernels of one walk
// window after another, read by the host once, at the file's end
struct StreamPos {
  unsigned long long at;    // where the next walk window's text begins, behind the file's first text byte
  unsigned long long kept;  // records whose text has a place
  unsigned long long rows;  // records met, skipped ones included
  uint32_t bad;             // a record outside its window, or a layout outside its block_size
  uint32_t over;            // a row's bytes had no room in the text
};

// the text bytes of the record at rec, of which `room` bytes are readable: l_seq + 1, or 0 for one that is skipped;
// *ok false: the record does not lie within `room`, or its fields not within its block_size.  QUAL: the qualities are
// counted into the layout as well (bam_rows.hip: plausible) — what the streaming form's text bound stands on.
template <bool QUAL>
__device__ __forceinline__ uint64_t rec_text_bytes(const uint8_t* __restrict__ rec, uint64_t room, uint32_t flag, bool* ok) {
  *ok = kRecHead <= room;
  if (!*ok) return 0;
  const uint32_t bs = ld32(rec), l_name = rec[12], n_cigar = ld32(rec + 16) & 0xFFFFu;
  const int32_t l_seq = (int32_t)ld32(rec + 20);
  *ok = l_seq >= 0 && l_name != 0 && 4 + (uint64_t)bs <= room &&
        32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (QUAL ? (uint64_t)l_seq : 0ull) <= bs;
  return *ok && !(flag & kSkip) ? (uint64_t)l_seq + 1 : 0;
}

// rows [0, n) by the waves of the grid, a wave a kept row: row r's bytes go to text[at + off[r], at + off[r + 1]), no byte
// at or beyond cap; rec_at(r) is the record
template <class RecAt>
__device__ __forceinline__ void write_rows(uint64_t n, const uint64_t* __restrict__ off, uint8_t* __restrict__ text, uint64_t at,
                                           uint64_t cap, uint32_t* over, RecAt rec_at) {
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
      if (a1 <= cap && at <= cap - a1) emit<kBases>(rec_at(r), a1 - a0, text + at + a0, lane);
      else if (lane == 0) *over = 1;
    }
  }
}

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
    bool ok = off <= stream_bytes;
    if (ok) out = rec_text_bytes<false>(stream + off, stream_bytes - off, flag[r], &ok);
    kept = out != 0;
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
  write_rows(n, off, text, at, cap, &tot->over, [&](uint64_t r) { return stream + rec_off[r]; });
}

// ---- the streaming form: the same two steps over one walk window's ring of compact rows (bam_rows.h: CompactRows), the
// count read from the row kernels' control block on the device, the text position from StreamPos.
// (cap + 1 entries: every entry from the window's count on is 0, so that the scan's entry cap is the window's total.)
// A record lies within its window when it begins no further in front of the buffer than the room there and ends at or
// before the walk window's end.
__global__ void __launch_bounds__(kBlock) k_bamstream_len(const uint8_t* __restrict__ win, int64_t front, int64_t end,
                                                          const int32_t* __restrict__ roff, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ n_rec, const uint32_t* __restrict__ anomaly,
                                                          uint32_t cap, uint64_t* __restrict__ len, StreamPos* pos) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r > cap) return;
  const uint32_t n = *anomaly ? 0u : (*n_rec < cap ? *n_rec : cap);  // (after an anomaly the ring is stale)
  uint64_t out = 0;
  if (r < n) {
    const int64_t o = roff[r];
    bool ok = o >= -front && o <= end;
    if (ok) out = rec_text_bytes<true>(win + o, (uint64_t)(end - o), flag[r], &ok);
    if (!ok) pos->bad = 1;
  }
  len[r] = out;
  const bool kept = out != 0;
  const uint64_t mask = __ballot(kept);  // one addition a wave
  if (kept && (threadIdx.x % kWave) == (uint32_t)__builtin_ctzll(mask)) atomicAdd(&pos->kept, (unsigned long long)__popcll(mask));
}

// off: the scan of k_bamstream_len's counts; the file's text begins at text[at], the window's pos->at behind that, which
// k_bamstream_next moves
__global__ void __launch_bounds__(kBlock) k_bamstream_write(const uint8_t* __restrict__ win, const int32_t* __restrict__ roff,
                                                            const uint32_t* __restrict__ n_rec, uint32_t cap,
                                                            const uint64_t* __restrict__ off, uint8_t* __restrict__ text,
                                                            uint64_t at, uint64_t text_cap, StreamPos* pos) {
  const uint32_t n = *n_rec < cap ? *n_rec : cap;  // (rows beyond the count have no bytes)
  write_rows(n, off, text, at + pos->at, text_cap, &pos->over, [&](uint64_t r) { return win + roff[r]; });
}

// one thread, behind k_bamstream_write: the text position and the record count move past the window
__global__ void k_bamstream_next(const uint64_t* __restrict__ off, uint32_t cap, const uint32_t* __restrict__ n_rec,
                                 const uint32_t* __restrict__ anomaly, StreamPos* pos) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || *anomaly) return;
  pos->at += off[cap];
  pos->rows += *n_rec;
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
  StreamPos* pos = nullptr;  // (the streaming form)
  Scratch tmp;               // (a piece of `all`)
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
  // what cannot be resident is known from the file's size: nothing is inflated to find it out
  {
    const uint64_t total = bam_->inflated_bytes(), need = total + 64 + (total / 36 + 2) * 52;  // (bam_rows.hip: BamRowsDevice::create)
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      *why = "the device cannot be used";
      return kGaveUp;
    }
    if (total / 36 + 1 >= (uint64_t)UINT32_MAX - 1) {
      did_not_fit_ = true;
      *reason = kBamReadsAnomaly;
      *anomaly = kRowsLimits;
      *why = "BAM rows: a file outside the row kernels' index widths";
      return kGaveUp;
    }
    if (need > std::min<uint64_t>(free_b / 2, resident_cap ? resident_cap : UINT64_MAX)) {
      did_not_fit_ = true;
      *reason = kBamReadsOverCap;
      *why = "the inflated BAM stream and its rows are over the cap";
      return kGaveUp;
    }
  }
  int refused = kResidentKept;
  rows_.reset(bam_->rows_on_device(window, anomaly, &w, true, resident_cap, &refused));
  windows_ = bam_->rows_windows();
  if (!rows_) {
    *reason = *anomaly == kRowsHip ? kBamReadsHip : kBamReadsAnomaly;
    *why = "BAM rows: " + w;
    return kGaveUp;
  }
  if (refused != kResidentKept || !rows_->stream_buffer() || !rows_->rows().rec_off) {
    did_not_fit_ = true;
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

// ---- the streaming form

void BamReadsDevice::drop_device() {
  work_.reset();
  rows_.reset();
}

BamReadsDevice::Result BamReadsDevice::stream_open(const ReadsInput& in, int device, size_t window, std::string* why) {
  const std::string name = in.path.empty() ? "(memory)" : in.path;
  drop_device();
  if (!bam_) {
    bam_.reset(new BamFile());
    std::string w;
    const bool opened = in.mem || in.path.empty() ? bam_->open_mem(in.mem, in.mem_n, &w) : bam_->open_path(in.path, &w);
    if (!opened) { *why = name + ": " + w; return kIoError; }
    bam_->set_window_bytes(window);
    bam_->set_inflate_device(device);
  }
  const uint64_t total = bam_->inflated_bytes();
  stream_bytes_ = total;
  payload_ = total > bam_->first_record() ? total - bam_->first_record() : 0;
  const uint64_t slots = bam_->inflate_device_bytes();  // (nothing is allocated before the caller has seen the sum)
  const size_t largest = bam_->largest_window();
  const size_t walk = window && window < largest ? window : largest;
  const size_t m = ring_entries_ = (size_t)BamRowsDevice::ring_capacity_of(walk) + 1;
  G2S_HIP_TRY_AS(hipSetDevice(device), (hip_fail(why, what_, e_), kGaveUp));
  G2S_HIP_TRY_AS(exclusive_scan_bytes<uint64_t>(m, &scan_bytes_), (hip_fail(why, what_, e_), kGaveUp));
  work_bytes_ = 2 * ((m * 8 + 255) & ~(size_t)255) + 256 + scan_bytes_;
  fixed_bytes_ = slots + BamRowsDevice::compact_bytes(walk) + work_bytes_;
  return kOk;
}

BamReadsDevice::Result BamReadsDevice::stream_run(uint8_t* d_text, uint64_t at, uint64_t cap, size_t window, int* reason,
                                                  int* anomaly, std::string* why) {
  *reason = kBamReadsHip;
  *anomaly = kRowsOk;
  // the arrays between the kernels, as stream_open counted them, and the position at the file's first text byte
  {
    const size_t arr = (ring_entries_ * 8 + 255) & ~(size_t)255;
    work_.reset(new Work());
    G2S_HIP_TRY_AS(work_->all.alloc(work_bytes_), (hip_fail(why, what_, e_), kGaveUp));
    work_->len = work_->all.as<uint64_t>();
    work_->off = (uint64_t*)(work_->all.as<uint8_t>() + arr);
    work_->pos = (StreamPos*)(work_->all.as<uint8_t>() + 2 * arr);
    work_->tmp.p = work_->all.as<uint8_t>() + 2 * arr + 256;
    work_->tmp.bytes = scan_bytes_;
    const StreamPos first{};
    G2S_HIP_TRY_AS(hipMemcpy(work_->pos, &first, sizeof first, hipMemcpyHostToDevice), (hip_fail(why, what_, e_), kGaveUp));
  }
  // one walk window's rows: lengths, their scan, the text, the position moved — enqueued behind the row kernels
  const RowsSink sink = [this, d_text, at, cap](const CompactRows& R, const uint8_t* d_win, size_t front, size_t end, std::string* why) -> bool {
    hipStream_t s = (hipStream_t)R.stream;
    const size_t m = (size_t)R.capacity + 1;
    if (m != ring_entries_) { *why = "the ring is not the one the streaming form planned for"; return false; }
    hipLaunchKernelGGL(k_bamstream_len, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_win, (int64_t)front,
                       (int64_t)end, R.off, R.flag, R.n_rec, R.anomaly, R.capacity, work_->len, work_->pos);
    G2S_HIP_TRY(hipGetLastError());
    G2S_HIP_TRY(exclusive_scan(work_->tmp, work_->len, work_->off, m, s));
    const unsigned waves_wanted = (R.capacity + kWave - 1) / kWave;
    const unsigned groups = std::max(1u, std::min((waves_wanted + kBlock / kWave - 1) / (kBlock / kWave), 256u * 16u));
    hipLaunchKernelGGL(k_bamstream_write, dim3(groups), dim3(kBlock), 0, s, d_win, R.off, R.n_rec, R.capacity,
                       (const uint64_t*)work_->off, d_text, at, cap, work_->pos);
    hipLaunchKernelGGL(k_bamstream_next, dim3(1), dim3(1), 0, s, (const uint64_t*)work_->off, R.capacity, R.n_rec, R.anomaly,
                       work_->pos);
    G2S_HIP_TRY(hipGetLastError());
    return true;
  };
  std::string w;
  rows_.reset(bam_->rows_on_device(window, anomaly, &w, false, 0, nullptr, &sink));
  windows_ = bam_->rows_windows();
  if (!rows_) {
    *reason = *anomaly == kRowsHip ? kBamReadsHip : kBamReadsAnomaly;
    *why = "BAM rows: " + w;
    return kGaveUp;
  }
  StreamPos pos{};  // (rows_on_device has waited for the stream)
  G2S_HIP_TRY_AS(hipMemcpy(&pos, work_->pos, sizeof pos, hipMemcpyDeviceToHost), (hip_fail(why, what_, e_), kGaveUp));
  if (pos.bad) {
    *reason = kBamReadsAnomaly;
    *anomaly = kRowsDeadLink;
    *why = "BAM text: a record outside its window";
    return kGaveUp;
  }
  if (pos.over) {
    *reason = kBamReadsOverCap;
    *why = "the BAM text outgrew what the cap left for it";
    return kGaveUp;
  }
  kept_ = pos.kept;
  rows_n_ = pos.rows;
  text_bytes_ = pos.at;
  *reason = kBamReadsKernels;
  return kOk;
}

}  // namespace g2s
