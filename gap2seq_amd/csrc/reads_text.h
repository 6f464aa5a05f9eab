// gap2seq_amd/csrc/reads_text.h — the graph build's text made from read files (reads_text.hip).
//
// For the sequences s0 ... s(n-1) of a list of FASTA/FASTQ (and BAM: bam_reads.h) files the build's text is s0 N s1 N ... s(n-1) N.  The device
// loader makes it in device memory from the files' raw bytes, a piece at a time, with the kernels k_fastx_* (the state
// machine of fastx_machine.h); gzip input is inflated on the way: BGZF members on the device (bgzf_inflate.h), any
// other gzip stream by zlib into the staging buffers — or, when asked for, chunk by chunk on the device too
// (gzip_inflate.h), zlib reading again what that route gives back.  The host loader (fastx.hpp) is the fallback and the
// authority.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fastx_machine.h"
#include "gzip_inflate.h"

namespace g2s {

// how a file's bytes were inflated
enum ReadsInflate : int { kInflateNone = 0, kInflateZlib = 1, kInflateDevice = 2, kInflateMixed = 3, kInflateDeviceGzip = 4 };

// who wrote the text of the BAM files among the read files (g2s_test_last_reads_bam), and when not the kernels, why
enum BamReadsReason : int {
  kBamReadsKernels = 0,   // k_bamreads_* or, streaming, k_bamstream_* (bam_reads.hip)
  kBamReadsNotAsked = 1,  // G2S_HOST_BUILD, G2S_HOST_READS=1, G2S_HOST_INFLATE=1, or no usable device
  kBamReadsAnomaly = 2,   // the row kernels gave the file back (bam_rows.h: RowsAnomaly says which)
  kBamReadsOverCap = 3,   // beyond half the free device memory, or G2S_BUILD_RESIDENT_CAP: stream, rows and text, and the
                          // streaming form's slots, rings and text as well (or its text outgrew what the limit left)
  kBamReadsHip = 4,       // an allocation or a HIP call failed
};

// What the process's last g2s_graph_build_files did to load its reads (g2s_test_last_reads_load, g2s_test_last_reads_bam).
struct ReadsLoadInfo {
  uint64_t files = 0, raw_bytes = 0, positions = 0, records = 0, pieces = 0, grows = 0;
  int on_device = 0;
  std::vector<int> inflate;  // per file: ReadsInflate
  // the BAM files among them: their number, the records kept and skipped, whether the kernels wrote their text
  uint64_t bam_files = 0, bam_kept = 0, bam_skipped = 0;
  int bam_kernels = 0, bam_reason = kBamReadsNotAsked, bam_anomaly = 0;
  // the streaming form (g2s_test_last_reads_bam_stream): the BAM files whose text it wrote, the walk windows they took,
  // the largest footprint counted against the limit (slots, candidates, ring, scan scratch and the text's capacity)
  uint64_t bam_streamed = 0, bam_stream_windows = 0, bam_stream_peak = 0;
  // the plain gzip files the chunked device inflate was tried on (gzip_inflate.h; g2s_test_last_reads_gzip): outcome is the
  // last file's that was given back to zlib, kGzDone when none was
  GzipStats gzip;
};

// one input of the loader: a file by name, or bytes in memory (the test hook)
struct ReadsInput {
  std::string path;
  const uint8_t* mem = nullptr;
  size_t mem_n = 0;
};

// A text resident on a device.  d_text has `capacity` bytes, at least device_text_bytes(T): what the key-range passes
// read, T rounded up to their tile plus their halo (solid_passes.h); the bytes from T to there are 'N'.  The owner frees
// d_text (free_device_text).
struct DeviceText {
  uint8_t* d_text = nullptr;
  uint64_t T = 0, capacity = 0;
  int device = -1;
};
// the bytes a text of T positions needs (solid_passes.h: tile padding and halo)
uint64_t device_text_bytes(uint64_t T);

enum ReadsLoadResult : int {
  kReadsOk = 0,
  kReadsGaveUp = 1,   // the device cannot be used or refused: *err says why; the host loader takes over
  kReadsIoError = 2,  // a file cannot be read, or is truncated or corrupt: *err names it
};

// The text of `inputs` (in order, the parser's state fresh for each) made on `device` in pieces of `piece` raw bytes
// (0: chosen by the files' sizes, 32 MiB at most);
// first_cap: the text buffer's first capacity in bytes when no bound is known (compressed input), 0 = the default.
// host_inflate: BGZF members go to zlib too.  On kReadsOk *out owns the text (also when T == 0).
// A BAM file of the list (bam_reads.h) gives its text through the kernels k_bamreads_* behind what the list has given so
// far, the text buffer sized from its count; `piece` is then its window, resident_cap (G2S_BUILD_RESIDENT_CAP, 0: none)
// lowers the bound of half the free device memory on its stream, rows and text.  With host_inflate its text is made by
// the host walk and copied up.  On kReadsGaveUp info->bam_reason / bam_anomaly say what a BAM file met.
// A BAM file that cannot be resident within the bound takes the streaming form (bam_reads.h) when everything that form
// holds fits the same bound; bam_stream (G2S_BUILD_BAM_STREAM) 1: the streaming form always, 0: never, -1: by that rule.
// out->capacity may then exceed device_text_bytes(T).
// device_gzip: a gzip file that is no BGZF file is inflated chunk by chunk on the device (gzip_inflate.h) and read again by
// zlib from its first byte when that route gives it back; not with host_inflate.
ReadsLoadResult load_reads_device(const std::vector<ReadsInput>& inputs, int device, size_t piece, uint64_t first_cap,
                                  bool host_inflate, DeviceText* out, ReadsLoadInfo* info, std::string* err,
                                  uint64_t resident_cap = 0, int bam_stream = -1, bool device_gzip = false);
void free_device_text(DeviceText* t);

// the machine of fastx_machine.h walked line by line on the host over one file's bytes: the text is appended to *out
void machine_text_host(const uint8_t* bytes, size_t n, std::string* out, uint64_t* records);

}  // namespace g2s
