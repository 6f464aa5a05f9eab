// gap2seq_amd/csrc/bam_reads.h — a BAM file as a read file of the graph build (bam_reads.hip).
//
// The definition (include/g2s.h).  A file is BAM when its bytes say so (fastx.hpp: is_bam), never by its name.  Every
// alignment record that is neither secondary (0x100) nor supplementary (0x800) contributes, mapped or not, in file
// order: its sequence as the read filter prints it (readfilter_gaps.hpp: append_bases — codes 1, 2, 4, 8 are A, C, G, T,
// every other code N, a reverse-strand record reverse-complemented back to the read as sequenced), followed by 'N'.  A
// kept record without bases gives its 'N' alone.  The file's text is these back to back.
//
// Host route (bam_reads_host): BamFile::for_each and append_bases; the authority and the fallback.
// Device route (BamReadsDevice), resident: the file is inflated on the device into one allocation with every record's offset and
// flag beside it (BamFile::rows_on_device, resident), and two kernels make the text from there —
//   k_bamreads_len    one thread a row: kept ? l_seq + 1 : 0 as a 64-bit count, the record's layout checked against the
//                     stream's end once more
//   (rocPRIM)         an exclusive 64-bit scan over n + 1 entries; entry n is the text's length, which sizes the text
//                     before anything is written
//   k_bamreads_write  a wave a kept row, the lanes over the row's output bytes (bam_decode.h, as bam_text.hip's k_decode)
// The caller (reads_text.hip: Loader::run_bam_file) owns the text buffer and places the file's text in it.
//
// The resident route holds the inflated stream (S bytes) and 52 bytes of rows for every 36 of them beside the text, all
// within half the free device memory (and G2S_BUILD_RESIDENT_CAP).  A file over that takes the streaming form, which is
// bounded by its text alone (G2S_BUILD_BAM_STREAM=1|0: always, never):
//   the file goes through the inflate's two slots window by window (BamFile::rows_on_device with a sink); the row
//   kernels leave of every whole record of a walk window its offset in the window buffer and its flag in a ring of the
//   walk window's capacity (bam_rows.h: CompactRows), and right behind them, on the same stream, before the slot is
//   written again —
//   k_bamstream_len    one thread a ring entry: the same count, the count of rows read from the row kernels' control
//                      block on the device, the record's layout checked against its window's extent; 0 beyond the count
//   (rocPRIM)          an exclusive 64-bit scan over capacity + 1 entries
//   k_bamstream_write  a wave a kept row, from the text position the device carries (StreamPos), every store checked
//                      against the text's capacity
//   k_bamstream_next   one thread: the position and the record count move past the window
//   The host does not wait for a window's kernels; it reads the position once, at the file's end.  Nothing of the inflated stream outlives its slot.
// The text is allocated once, before the first window, from a bound: a kept record of l_seq bases takes at least
// 36 + 1 + ceil(l_seq / 2) + l_seq stream bytes (the fixed fields, the name's terminator, bases, qualities — what
// bam_rows.hip's plausible() enforces and k_bamstream_len checks again), so its l_seq + 1 text bytes are at most two
// thirds of them: capacity = device_text_bytes(have + min(2 * S / 3, what the limit leaves)), S the inflated bytes
// behind the header.  Known cost: the slack behind the text stays allocated through the count — 2/3 of the stream at
// the worst, about 1.45 times the text for 150-base reads with typical names and tags.
// The fixed footprint, independent of the file's size, for windows of w bytes (w' the largest window of whole members,
// at most max(w, 64 KiB), of m members; the front F is 256 KiB):
//   the two slots     2 * (F + w' + 64 + staged input (at most w' + 21 * m + 16) + 28 * (m + 1))
//   candidates, ring  26 * (w / 36 + 65) + 4 * (w / 4096 + 2) + 160
//   lengths, scan     16 * (w / 36 + 66) + 768 + rocPRIM's scratch for that many entries
// which 2 * (F + 2 * w' + 64 * (m + 1)) + 64 * (w / 36 + 66) + 64 KiB bounds from above.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "reads_text.h"

namespace g2s {

class BamFile;
class BamRowsDevice;

// the host route.  The kept records' sequences are appended to *seqs; *skipped counts the records left out, *raw_bytes
// the inflated stream.  False: *err names the file (a member that does not inflate, a cut record, a header that does
// not parse).
bool bam_reads_host(const ReadsInput& in, std::vector<std::string>* seqs, uint64_t* skipped, uint64_t* raw_bytes, std::string* err);

// One BAM file on its way through the device route: prepare() inflates it, makes the rows, counts and scans; the caller
// then knows text_bytes() and gives write() the place.  The resident stream and the rows go with the object.
class BamReadsDevice {
 public:
  enum Result : int { kOk = 0, kGaveUp = 1, kIoError = 2 };
  BamReadsDevice();
  ~BamReadsDevice();
  BamReadsDevice(const BamReadsDevice&) = delete;
  BamReadsDevice& operator=(const BamReadsDevice&) = delete;
  // window: the inflated bytes of a window of the inflate and of the row kernels' walk (0: the reader's own, 32 MiB);
  // resident_cap: G2S_BUILD_RESIDENT_CAP (0: half the free device memory alone).  kGaveUp: *reason (BamReadsReason, with
  // *anomaly a RowsAnomaly when that is the reason) and *why; kIoError: *why names the file.
  Result prepare(const ReadsInput& in, int device, size_t window, uint64_t resident_cap, int* reason, int* anomaly,
                 std::string* why);
  uint64_t text_bytes() const { return text_bytes_; }
  uint64_t kept() const { return kept_; }
  uint64_t skipped() const { return rows_n_ - kept_; }
  uint64_t stream_bytes() const { return stream_bytes_; }
  uint64_t windows() const { return windows_; }
  uint64_t resident_bytes() const { return resident_bytes_; }  // device memory held: the stream and the rows
  void* stream() const;                                        // the hipStream_t the kernels run on
  // after a prepare() that gave up: the file cannot be resident (over the cap, no memory for it, more than 2^32
  // records), which is the streaming form's case
  bool resident_did_not_fit() const { return did_not_fit_; }
  // ---- the streaming form.  stream_open (after a prepare() or alone) opens the file if need be, frees what a
  // prepare() left on the device, and says what the form will hold: stream_payload() inflated bytes behind the header,
  // which bound the text, and stream_fixed_bytes() of device memory beside the text — a sum, nothing is allocated for
  // it.  stream_run then takes that memory and writes the text to d_text[at, at + text_bytes()), no byte at or beyond
  // cap (the text's bound, not the buffer's size), and waits for it; kept(), skipped(), windows() as for
  // the resident route.  kGaveUp: *reason — kBamReadsOverCap when the text outgrew cap — *anomaly and *why.
  void drop_device();
  Result stream_open(const ReadsInput& in, int device, size_t window, std::string* why);
  uint64_t stream_payload() const { return payload_; }
  uint64_t stream_fixed_bytes() const { return fixed_bytes_; }
  Result stream_run(uint8_t* d_text, uint64_t at, uint64_t cap, size_t window, int* reason, int* anomaly, std::string* why);
  // the text to d_text[at, at + text_bytes()), no byte at or beyond cap; waits for it.  False: *why.
  bool write(uint8_t* d_text, uint64_t at, uint64_t cap, std::string* why);

 private:
  bool count(bool* bad, std::string* why);
  struct Work;  // (bam_reads.hip) the device arrays between the two kernels
  std::unique_ptr<BamFile> bam_;
  std::unique_ptr<BamRowsDevice> rows_;
  std::unique_ptr<Work> work_;
  uint64_t text_bytes_ = 0, kept_ = 0, rows_n_ = 0, stream_bytes_ = 0, windows_ = 0, resident_bytes_ = 0;
  uint64_t payload_ = 0, fixed_bytes_ = 0;
  size_t work_bytes_ = 0, scan_bytes_ = 0, ring_entries_ = 0;  // the arrays between the streaming kernels, as planned
  bool did_not_fit_ = false;
};

}  // namespace g2s
