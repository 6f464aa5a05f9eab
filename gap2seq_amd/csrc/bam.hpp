// gap2seq_amd/csrc/bam.hpp — a BAM reader for the read filter (readfilter.cpp): BGZF blocks
// inflated with zlib, several blocks at a time on a few threads — or on the GPU (set_inflate_device,
// bgzf_inflate.hip), a window ahead of the records being walked — records handed to a callback
// in file order.  It replaces the part of htslib the reference's ReadFilter uses
// (/root/reference/src/ReadFilter.cpp:66-101 io_t, :176-222 sam_iterator): open, header,
// "every record" and "records overlapping [beg, end) of one reference".  No index is read:
// the reference's run makes two passes over the whole file anyway (:225-241 count_reads,
// :313-323 find_mates), so region queries are answered by the same kind of pass with htslib's
// overlap test (tid equal, pos < end, end position > beg).
// Formats: SAM/BAM specification, sections 4.1 (BGZF) and 4.2 (BAM).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "bam_rows.h"

namespace g2s {

class BgzfDevice;

enum : uint32_t {
  BAM_PAIRED = 1, BAM_UNMAPPED = 4, BAM_MATE_UNMAPPED = 8, BAM_REVERSE = 16, BAM_READ1 = 64, BAM_READ2 = 128,
  BAM_SECONDARY = 0x100, BAM_SUPPLEMENTARY = 0x800
};

// one alignment record, pointing into the reader's buffer (valid during the callback only)
struct BamRec {
  int32_t ref_id, pos, next_ref_id, next_pos, tlen, l_seq;
  uint32_t flag, n_cigar, l_name;
  uint8_t mapq;
  const char* name;        // l_name bytes, NUL terminated by the format
  const uint8_t* cigar;    // n_cigar little-endian words: length << 4 | op
  const uint8_t* seq;      // 4-bit codes "=ACMGRSVTWYHKDBN", high nibble first
  // htslib's bam_endpos: position after the last reference base the alignment covers; an unmapped record
  // or one whose CIGAR consumes no reference counts as one base
  int64_t end_pos() const {
    int64_t rlen = 0;
    if (!(flag & BAM_UNMAPPED))
      for (uint32_t i = 0; i < n_cigar; i++) {
        uint32_t w;
        memcpy(&w, cigar + 4 * (size_t)i, 4);
        const uint32_t op = w & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4;  // M D N = X
      }
    return (int64_t)pos + (rlen ? rlen : 1);
  }
  uint8_t base4(int32_t i) const { return (uint8_t)((seq[i >> 1] >> ((~i & 1) << 2)) & 15); }
};

class BamFile {
 public:
  BamFile() {}
  ~BamFile();
  BamFile(const BamFile&) = delete;
  BamFile& operator=(const BamFile&) = delete;
  // map the file / adopt the caller's bytes, index the BGZF blocks, read the header
  bool open_path(const std::string& path, std::string* err);
  bool open_mem(const void* bytes, size_t n, std::string* err);
  const std::vector<std::string>& ref_names() const { return ref_names_; }
  int ref_id(const std::string& name) const;  // -1 when the header has no such reference
  // every record in file order; stops early (returning true) when fn returns false.  False = broken file.
  bool for_each(const std::function<bool(const BamRec&)>& fn, std::string* err) const;
  void set_threads(int t) { threads_ = t < 1 ? 1 : t; }
  // inflated bytes a window (whole members, one at the least) of the passes that follow; 0: G2S_BAM_CHUNK, else 32 MiB
  void set_window_bytes(size_t n) { window_bytes_ = n; }
  size_t blocks() const { return blk_off_.size(); }
  // Where for_each / read_all inflate.  device >= 0: the members of a window are inflated by g2s_bgzf_inflate on that
  // device while the window before is being walked; a device that refuses (no usable gfx950, an allocation or a HIP
  // call that fails) hands the file to the host path for good, silently (G2S_DEBUG=1 prints why).  -1: zlib on host
  // threads.  A corrupt member is the same error on either.
  void set_inflate_device(int device);
  // Pass A of the batched filter without a walk (bam_rows.h): the rows of every record made by kernels on the inflate
  // device from the windows while they lie in device memory, `walk_window` bytes at a time (0: a whole window of
  // inflated members).  The caller owns the result.  Null: *anomaly (bam_rows.h: RowsAnomaly) and *why say what
  // stood in the way; nothing is left in flight, no inflate statistics were counted, and for_each is the way to go on.
  // `resident` (one-pass mode): the inflated stream stays in one device allocation of the result, with every record's
  // offset in it (BamRowsDevice::stream_buffer, DeviceRows::rec_off), when it fits the cap (bam_rows.h: ResidentAsk;
  // resident_cap 0: half the free device memory alone); *resident_refused (bam_rows.h: ResidentRefused) says when it did
  // not, and the rows are then made the two-slot way.
  // `sink` (the read route's streaming form, not with `resident`): the two-slot way with compact rows (bam_rows.h:
  // CompactRows) handed to *sink behind every walk window's row kernels, before the window's slot is written again;
  // no array of the result grows with the file, and a file may hold more than 2^32 records.
  // `store` (with `resident`; bam_store.h): the store route between the two — when the whole stream is refused as over the
  // cap (mode -1), or in any case (mode 1), and the capacities planned from the file's sample fit the same cap, the
  // windows go through the two slots and every record's head, name and packed bases are copied to one device allocation
  // of the result behind the row kernels; stream_buffer() and rec_off are then the store's.  A planned capacity that
  // proves too small ends the pass with the anomaly kRowsPlanRows or kRowsPlanStore.  store_report() says what happened.
  struct StoreAsk {
    int mode = -1;          // -1 when the whole stream is over the cap, 1 always, 0 never
    uint64_t sample = 0;    // the sample's bytes behind the header; 0: kStoreSampleBytes
    bool worst_case = false;  // tests: no sample, the capacities that cannot overflow (P / 36 + 1 rows, P bytes)
  };
  BamRowsDevice* rows_on_device(size_t walk_window, int* anomaly, std::string* why, bool resident = false,
                                uint64_t resident_cap = 0, int* resident_refused = nullptr, const RowsSink* sink = nullptr,
                                const StoreAsk* store = nullptr) const;
  uint64_t rows_windows() const { return rows_windows_; }  // walk windows of the last rows_on_device
  const StoreReport& store_report() const { return store_report_; }  // the store route in the last rows_on_device
  // The plan of the store route's capacities (bam_store.h: store_plan) from the records that begin in the first `sample`
  // inflated bytes behind the header (0: kStoreSampleBytes; the whole file when it is smaller), inflated here with zlib.
  // False: *err (a member of the sample did not inflate).
  bool store_sample(uint64_t sample, StorePlan* plan, std::string* err) const;
  // the host model of the store (tests): every record compacted by bam_store::append_record, and where each begins
  bool store_on_host(std::vector<uint8_t>* store, std::vector<uint64_t>* rec_off, std::string* err) const;
  // the file's inflated bytes (the members' ISIZE fields summed) and the offset of the first record among them
  uint64_t inflated_bytes() const;
  uint64_t first_record() const { return first_rec_; }
  // the inflated bytes of the largest window of whole members; *staged, *members, *inflated (any may be null): the
  // largest staged deflate bytes, member count and inflated bytes of a window, each over all windows
  size_t largest_window(size_t* staged = nullptr, size_t* members = nullptr, size_t* inflated = nullptr) const;
  // the device memory the inflate's two slots take for this file's windows (nothing is allocated to say so)
  uint64_t inflate_device_bytes() const;
  // test paths (g2s_test_bgzf_inflate): the host path with inflate_core.h in zlib's place; any BGZF file, no BAM header
  void set_inflate_core(bool on) { use_core_ = on; }
  bool open_bgzf(const void* bytes, size_t n, std::string* err);
  // the whole inflated stream; false: *err, and *bad_block = the corrupt member when that is the error (else -1)
  bool read_all(std::vector<uint8_t>* out, std::string* err, int64_t* bad_block) const;
  // what the refills since reset_inflate_stats() did: members and bytes in and out, the time inside refill (with the
  // device: what the walk waited), and whether every window came from the device
  struct InflateStats {
    uint64_t members = 0, bytes_in = 0, bytes_out = 0, device_windows = 0, host_windows = 0;
    double ms_refill = 0;
  };
  const InflateStats& inflate_stats() const { return stats_; }
  void reset_inflate_stats() const { stats_ = InflateStats(); }

 private:
  bool index_blocks(std::string* err);
  bool read_header(std::string* err);
  struct Stream;
  const uint8_t* data_ = nullptr;
  size_t size_ = 0;
  void* map_ = nullptr;
  size_t map_len_ = 0;
  std::vector<uint64_t> blk_off_;     // offset of each BGZF block
  std::vector<uint32_t> blk_csize_;   // its size in the file
  std::vector<uint32_t> blk_isize_;   // and inflated
  std::vector<uint16_t> blk_dataoff_; // offset of the deflate stream inside the block
  std::vector<std::string> ref_names_;
  uint64_t first_rec_ = 0;            // inflated offset of the first alignment record
  int threads_ = 4;
  size_t window_bytes_ = 0;
  bool use_core_ = false;
  int inflate_device_ = -1;
  BgzfDevice* device_buffers() const;           // made at the first device refill, kept for the passes that follow
  mutable std::shared_ptr<BgzfDevice> dev_;
  mutable bool dev_refused_ = false;
  mutable InflateStats stats_;
  mutable uint64_t rows_windows_ = 0;
  mutable StoreReport store_report_;
};

}  // namespace g2s
