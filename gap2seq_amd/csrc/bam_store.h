// gap2seq_amd/csrc/bam_store.h — the store route of the batched read filter's one-pass mode (bam_store.hip): for a file
// whose whole inflated stream does not fit the device, pass A keeps of every record only what pass B reads — the head,
// the name and the packed bases — in one device allocation, the store, written window by window behind the row kernels
// while the window still lies in its inflate slot.  Pass B (bam_text.h) reads the store as it reads the resident stream.
//
// A stored record is itself a well-formed BAM record: the 36 head bytes with block_size rewritten to
// 32 + l_name + ceil(l_seq / 2) and n_cigar_op (bytes 16-17) rewritten to 0, every other field as it was; then the
// l_name name bytes (inner NULs included); then the ceil(l_seq / 2) packed base bytes.  Records lie back to back, with
// no alignment.  CIGAR, qualities and tags are not kept.  A stored record is never longer than its source, whose layout
// the row kernels have checked (bam_rows.hip: plausible).
// This header is compiled for host and device: the layout's arithmetic, the host model of one record, and the plan of
// the two capacities.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define G2S_STORE_HD __host__ __device__
#else
#define G2S_STORE_HD
#endif

namespace g2s {
namespace bam_store {

constexpr uint32_t kHead = 36;  // block_size and the 32 fixed bytes

// the bytes a record with this name and read length takes in the store
G2S_STORE_HD inline uint64_t stored_bytes(uint32_t l_name, uint64_t l_seq) { return (uint64_t)kHead + l_name + (l_seq + 1) / 2; }
// byte i < 36 of the stored head, from the source head's byte and the stored size
G2S_STORE_HD inline uint8_t head_byte(uint32_t i, uint8_t src, uint64_t stored) {
  if (i < 4) return (uint8_t)((stored - 4) >> (8 * i));  // block_size
  if (i == 16 || i == 17) return 0;                      // n_cigar_op
  return src;
}

// The host model: the record at `rec` (its block_size field first; the caller has checked its layout as
// BamFile::for_each does) compacted to the end of *out.
inline void append_record(const uint8_t* rec, std::vector<uint8_t>* out) {
  const uint32_t l_name = rec[12], n_cigar = (uint32_t)rec[16] | (uint32_t)rec[17] << 8;
  uint32_t l_seq;
  memcpy(&l_seq, rec + 20, 4);
  const uint64_t stored = stored_bytes(l_name, l_seq);
  for (uint32_t i = 0; i < kHead; i++) out->push_back(head_byte(i, rec[i], stored));
  out->insert(out->end(), rec + kHead, rec + kHead + l_name);
  const uint8_t* seq = rec + kHead + l_name + 4 * (size_t)n_cigar;
  out->insert(out->end(), seq, seq + ((size_t)l_seq + 1) / 2);
}

}  // namespace bam_store

// ---- the capacities, planned from a sample: neither the record count nor the stored bytes are known before the pass, and
// their worst case is the whole stream again.  The sample is the records that begin in the first sample bytes behind
// the header: r records over z bytes with c stored bytes.
struct StorePlan {
  uint64_t sample_records = 0, sample_bytes = 0, sample_stored = 0;  // r, z, c
  uint64_t rows_cap = 0, store_cap = 0;
  uint64_t need = 0;  // 52 * (rows_cap + 1) + store_cap: what grows with the file, counted against the bound
};
constexpr uint64_t kStoreSampleBytes = (uint64_t)1 << 20;
// With P the inflated bytes behind the header:
//   rows_cap  = min(P / 36 + 1, ceil(1.25 * r / z * P) + 64)
//   store_cap = min(P,          ceil(1.25 * c / z * P) + 4096)
// and the additive terms alone for a sample without records.  The factor 1.25 is a design constant, no measurement: a
// capacity that turns out too small is a clean way out (kTextStoreOverflow), not an error.
inline StorePlan store_plan(uint64_t P, uint64_t r, uint64_t z, uint64_t c) {
  StorePlan p;
  p.sample_records = r, p.sample_bytes = z, p.sample_stored = c;
  auto scaled = [&](uint64_t x) -> uint64_t {  // ceil(5 x P / (4 z)), saturating
    if (!z || !x) return 0;
    const unsigned __int128 q = ((unsigned __int128)5 * x * P + (unsigned __int128)4 * z - 1) / ((unsigned __int128)4 * z);
    return q > (unsigned __int128)(UINT64_MAX >> 1) ? UINT64_MAX >> 1 : (uint64_t)q;
  };
  const uint64_t rows = scaled(r) + 64, store = scaled(c) + 4096;
  p.rows_cap = rows < P / 36 + 1 ? rows : P / 36 + 1;
  p.store_cap = store < P ? store : P;
  p.need = 52 * (p.rows_cap + 1) + p.store_cap;
  return p;
}

// what a pass A in store form did (BamFile::store_report; g2s_test_last_filter_store)
struct StoreReport {
  int used = 0;      // 1: the pass ended with the store and its rows on the device
  int overflow = 0;  // 0 none, 1 the planned rows, 2 the planned store
  uint64_t records = 0, store_bytes = 0;  // what the store holds (also what it had taken when it overflowed)
  uint64_t store_cap = 0, rows_cap = 0, device_bytes = 0;  // the plan, and its need
};

// The store on the device (bam_store.hip).  BamRowsDevice owns one in store form and calls window() behind the row
// kernels of every walk window; the kernels read the walk window's record count, its first row and the anomaly word
// from the row kernels' control block, all on the device, and the host waits for no window.
class BamStoreDevice {
 public:
  // store_cap bytes and the arrays for walk windows of at most ring_cap records, on `stream`.  Null: *why (an
  // allocation or a HIP call failed).
  static BamStoreDevice* create(int device, void* stream, uint64_t store_cap, uint64_t rows_cap, uint32_t ring_cap, std::string* why);
  ~BamStoreDevice();
  BamStoreDevice(const BamStoreDevice&) = delete;
  BamStoreDevice& operator=(const BamStoreDevice&) = delete;
  // One walk window, enqueued: rec_off[*row_base + i] for i < *n_rec holds record i's offset relative to d_win (as an
  // int64; negative: carried in front, at most `front` bytes) and receives its offset in the store; the walk window ends
  // `end` bytes behind d_win.
  bool window(const uint8_t* d_win, size_t front, size_t end, const uint32_t* n_rec, const uint64_t* row_base,
              const uint32_t* anomaly, uint64_t* rec_off, std::string* why);
  // the position and the overflow word, once, behind everything enqueued (the caller has waited for the stream)
  bool finish(uint64_t* used_bytes, uint64_t* records, bool* overflow, bool* bad, std::string* why);
  uint8_t* buffer() const { return store_; }
  uint64_t capacity() const { return store_cap_; }

 private:
  BamStoreDevice() {}
  struct Buffers;
  Buffers* buf_ = nullptr;
  int device_ = -1;
  void* stream_ = nullptr;
  uint8_t* store_ = nullptr;
  uint64_t store_cap_ = 0, rows_cap_ = 0;
  uint32_t ring_cap_ = 0;
};

}  // namespace g2s
