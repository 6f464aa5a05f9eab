// gap2seq_amd/csrc/bam_rows.h — pass A of the batched read filter on the device (bam_rows.hip): the rows of
// readfilter_gaps.hpp's FilterRows made by kernels from the inflated windows while they lie in device memory.
// bam.cpp (BamFile::rows_on_device) hands the windows over; readfilter_gpu.hip's joins read the rows where they are.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "bam_store.h"

namespace g2s {

// why a pass gave up its device rows (g2s_test_last_filter_rows); the host walk then runs and is the authority
enum RowsAnomaly : int {
  kRowsOk = 0,
  kRowsDeadLink = 1,   // a record of the chain points at an offset that can be no record (or the head itself cannot)
  kRowsOverflow = 2,   // more candidates in a window than its capacity
  kRowsCarry = 3,      // a cut record's head longer than the room in front of a window
  kRowsWrongEnd = 4,   // the chain does not end at the stream's end
  kRowsHip = 5,        // an allocation or a HIP call failed
  kRowsHash = 6,       // name_hash.h is not this build's std::hash<std::string>
  kRowsCorrupt = 7,    // a member did not inflate
  kRowsLimits = 8,     // a file outside the kernels' index widths, or a header that does not end in the first window
  // the store route (bam_store.h) alone: a capacity planned from the file's sample was too small.  No fault of the
  // file's: the caller runs pass A again the two-pass way (bam_text.h: kTextStoreOverflow)
  kRowsPlanRows = 9,   // more records than the planned rows
  kRowsPlanStore = 10, // more stored bytes than the planned store
};

// rows in device memory, in file order; the arrays belong to the BamRowsDevice that made them
struct DeviceRows {
  int32_t *ref_id = nullptr, *pos = nullptr;
  int64_t* end = nullptr;
  uint32_t* flag = nullptr;
  uint64_t *h_own = nullptr, *h_mate = nullptr;  // (the joins replace them by their bits, in place)
  uint64_t* rec_off = nullptr;  // one-pass mode: every record's offset in the resident inflated stream, or in the store (else null)
  uint64_t n = 0;
  int64_t max_span = 1;
  int32_t read_length = 0;
};

// One-pass mode (bam_text.h): what pass A is asked to keep, and why it did not
struct ResidentAsk {
  uint64_t bytes = 0;  // the inflated stream, whole; 0: nothing is kept
  uint64_t cap = 0;    // G2S_FILTER_RESIDENT_CAP; 0: half the free device memory alone
  // The store route (bam_store.h), between "the whole stream is kept" and "nothing is kept".  store: -1 it is taken when
  // the whole stream is refused as over the cap, 1 it is taken even when the whole stream would fit, 0 never.  plan: the
  // two capacities, asked for only when the route is about to be taken (the caller inflates the file's sample for it);
  // false: no plan, no store.  The plan's need must fit the same bound.
  int store = 0;
  std::function<bool(StorePlan*)> plan;
};
enum ResidentRefused : int { kResidentKept = 0, kResidentOverCap = 1, kResidentNoMemory = 2 };

// The compact rows of the read route's streaming form (bam_reads.h): of every whole record of one walk window its
// offset relative to the window buffer's first byte (negative: a record carried in front of it) and its flag, in file
// order, in a ring of one walk window's capacity that the next walk window overwrites.  All device memory; *n_rec and
// *anomaly are the row kernels' control words, read on the device (after an anomaly the ring is stale).
struct CompactRows {
  const int32_t* off = nullptr;
  const uint32_t* flag = nullptr;
  const uint32_t* n_rec = nullptr;
  const uint32_t* anomaly = nullptr;
  uint32_t capacity = 0;  // entries of off / flag
  void* stream = nullptr;  // the hipStream_t the row kernels run on
};
// what consumes a walk window's compact rows: called behind the row kernels of every walk window, it enqueues its own
// kernels on the same stream, so that they have run before the window's slot is written again.  d_win: the window
// buffer's first byte, with `front` readable bytes in front of it; the walk window ends `end` bytes behind it.
using RowsSink = std::function<bool(const CompactRows& rows, const uint8_t* d_win, size_t front, size_t end, std::string* why)>;

class BamRowsDevice {
 public:
  // Kernels on `stream` (a hipStream_t: the reader's own, behind its inflate kernel) for windows of at most max_window
  // bytes, walked `walk_window` bytes at a time, each with `front` bytes of room in front; at most cap_rows rows;
  // references [0, n_ref); the first record at offset first_head of the first window.  Null: *why.
  // `ask` (may be null): one device allocation for the whole inflated stream and an offset per row beside the rows, taken
  // only when stream and rows fit within half the free device memory (and ask->cap).  When they do not, or the
  // allocation fails, the object is made without them and *resident_refused says which.
  // The store route (ask->store, ask->plan): in place of the whole stream a BamStoreDevice of the planned capacity, rows of
  // the planned count in place of cap_rows, and window() runs the store's kernels behind the row kernels of every walk
  // window: k_rec<true> leaves a record's offset in its window in rec_off, and the store's copy kernel replaces it by the
  // record's offset in the store.  The windows are then handed over the two-slot way (carry(), not advance()).
  // `sink` (may be null; not together with `ask`): the compact form — no whole-file arrays are made, cap_rows does not
  // apply, every walk window's rows go to the ring and then to *sink; rows() stays empty but for n.
  static BamRowsDevice* create(int device, void* stream, size_t max_window, size_t walk_window, size_t front,
                               uint64_t cap_rows, int32_t n_ref, uint64_t first_head, std::string* why,
                               const ResidentAsk* ask = nullptr, int* resident_refused = nullptr,
                               const RowsSink* sink = nullptr);
  // the device bytes create() takes in the compact form for walk windows of `walk_window` bytes
  static uint64_t compact_bytes(size_t walk_window);
  static uint32_t ring_capacity_of(size_t walk_window);  // the ring's entries
  ~BamRowsDevice();
  BamRowsDevice(const BamRowsDevice&) = delete;
  BamRowsDevice& operator=(const BamRowsDevice&) = delete;
  // the walk windows of one inflated window of `bytes` bytes at d_win (a device pointer), from offset `start`: enqueued
  // (win_off: d_win's offset in the resident stream, for DeviceRows::rec_off)
  bool window(const uint8_t* d_win, size_t start, size_t bytes, std::string* why, uint64_t win_off = 0);
  // the cut record's head moved in front of the next window's buffer: enqueued
  bool carry(const uint8_t* d_win, size_t bytes, uint8_t* d_next_win, std::string* why);
  // the same step between two windows of the resident stream, whose (word aligned) bases lie `step` bytes apart, the
  // first ending win_end bytes behind its base: nothing to copy, the head moves: enqueued
  bool advance(size_t win_end, size_t step, std::string* why);
  // the resident stream (null without one-pass mode) and its size; in store form the store and, after finish(), its
  // used bytes: a stream of well-formed records either way
  uint8_t* stream_buffer() const { return stream_buf_; }
  uint64_t stream_bytes() const { return stream_bytes_; }
  bool store_form() const { return store_ != nullptr; }
  const StoreReport& store_report() const { return report_; }  // (store form: the plan from create(), the rest from finish())
  int device() const { return device_; }
  void* stream() const { return stream_; }
  // the end of the stream behind a last window of last_bytes bytes: waits, and reads the counts down.  False: a HIP
  // call failed (*why).  *anomaly: kRowsOk, or what the kernels met.
  bool finish(size_t last_bytes, int* anomaly, std::string* why);
  // the first m rows copied to the host (tests)
  bool download(uint64_t m, int32_t* ref_id, int32_t* pos, int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate,
                std::string* why) const;
  // store form, after finish(): the store's used bytes and every record's offset in it, copied to the host (tests)
  bool download_store(std::vector<uint8_t>* store, std::vector<uint64_t>* rec_off, std::string* why) const;
  const DeviceRows& rows() const { return rows_; }
  uint64_t windows() const { return windows_; }
  uint64_t candidates() const { return candidates_; }

 private:
  BamRowsDevice() {}
  int device_ = -1;
  void* stream_ = nullptr;
  size_t walk_ = 0, front_ = 0;
  uint32_t cap_cand_ = 0, max_tiles_ = 0;
  uint64_t cap_rows_ = 0;
  int32_t n_ref_ = 0;
  DeviceRows rows_;
  struct Buffers;  // (bam_rows.hip) the device allocations, rows_' arrays and stream_buf_ among them
  Buffers* buf_ = nullptr;
  uint64_t windows_ = 0, candidates_ = 0;
  uint8_t* stream_buf_ = nullptr;
  uint64_t stream_bytes_ = 0;
  RowsSink sink_;  // (compact form)
  bool compact_ = false;
  BamStoreDevice* store_ = nullptr;  // (store form; owned)
  StoreReport report_;
};

}  // namespace g2s
