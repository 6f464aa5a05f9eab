// gap2seq_amd/csrc/bam_reads.h — a BAM file as a read file of the graph build (bam_reads.hip).
//
// The definition (include/g2s.h).  A file is BAM when its bytes say so (fastx.hpp: is_bam), never by its name.  Every
// alignment record that is neither secondary (0x100) nor supplementary (0x800) contributes, mapped or not, in file
// order: its sequence as the read filter prints it (readfilter_gaps.hpp: append_bases — codes 1, 2, 4, 8 are A, C, G, T,
// every other code N, a reverse-strand record reverse-complemented back to the read as sequenced), followed by 'N'.  A
// kept record without bases gives its 'N' alone.  The file's text is these back to back.
//
// Host route (bam_reads_host): BamFile::for_each and append_bases; the authority and the fallback.
// Device route (BamReadsDevice): the file is inflated on the device into one allocation with every record's offset and
// flag beside it (BamFile::rows_on_device, resident), and two kernels make the text from there —
//   k_bamreads_len    one thread a row: kept ? l_seq + 1 : 0 as a 64-bit count, the record's layout checked against the
//                     stream's end once more
//   (rocPRIM)         an exclusive 64-bit scan over n + 1 entries; entry n is the text's length, which sizes the text
//                     before anything is written
//   k_bamreads_write  a wave a kept row, the lanes over the row's output bytes (bam_decode.h, as bam_text.hip's k_decode)
// The caller (reads_text.hip: Loader::run_bam_file) owns the text buffer and places the file's text in it.
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
  // the text to d_text[at, at + text_bytes()), no byte at or beyond cap; waits for it.  False: *why.
  bool write(uint8_t* d_text, uint64_t at, uint64_t cap, std::string* why);

 private:
  bool count(bool* bad, std::string* why);
  struct Work;  // (bam_reads.hip) the device arrays between the two kernels
  std::unique_ptr<BamFile> bam_;
  std::unique_ptr<BamRowsDevice> rows_;
  std::unique_ptr<Work> work_;
  uint64_t text_bytes_ = 0, kept_ = 0, rows_n_ = 0, stream_bytes_ = 0, windows_ = 0, resident_bytes_ = 0;
};

}  // namespace g2s
