// gap2seq_amd/csrc/bam_text.h — pass B of the batched read filter on the device (bam_text.hip), for one-pass mode: the
// bases, names and FASTA text of the records the joins selected, gathered and decoded from the inflated stream pass A
// left in device memory (bam_rows.h: BamRowsDevice::stream_buffer, DeviceRows::rec_off) — or from the store of compacted
// records it left there (bam_store.h), which reads the same.  No inflate, no host walk.
// What it makes is what the host walk of pass B makes (readfilter_gaps.cpp: pass_b_host), array for array.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "bam_rows.h"

#if defined(__HIPCC__)
#define G2S_TEXT_HD __host__ __device__
#else
#define G2S_TEXT_HD
#endif

namespace g2s {

// g2s_test_last_filter_text's `reason`: why pass B of a batched call did not run on the device
enum TextReason : int {
  kTextOnDevice = 0,    // it did
  kTextNotAsked = 1,    // one-pass mode was not asked for (g2s_filter_set_one_pass, G2S_FILTER_ONE_PASS)
  kTextNoDeviceRows = 2,  // pass A's rows were not made on the device: no device, a switch, a pass-A anomaly
  kTextOverCap = 3,     // stream and rows beyond half the free device memory, or G2S_FILTER_RESIDENT_CAP
  kTextFailed = 4,      // an allocation or a HIP call failed, in pass A's resident buffer or in pass B
  kTextStoreOverflow = 5,  // the store route (bam_store.h): a capacity planned from the sample was too small; three passes
};

// A base as the filter prints it (readfilter_gaps.hpp: append_bases): the 4-bit codes 1, 2, 4, 8 are A, C, G, T, every
// other code is N; a reverse-strand record's bases are complemented (and read from its end by the caller).
G2S_TEXT_HD inline char base_char(uint32_t code, bool reverse) {
  // 16 characters as two words of eight, code 0 (and 8) in the low byte
  const uint64_t fwd_lo = 0x4E4E4E474E434100ull | 'N', fwd_hi = 0x4E4E4E4E4E4E4E00ull | 'T';
  const uint64_t rev_lo = 0x4E4E4E434E475400ull | 'N', rev_hi = 0x4E4E4E4E4E4E4E00ull | 'A';
  const uint64_t w = reverse ? (code & 8u ? rev_hi : rev_lo) : (code & 8u ? fwd_hi : fwd_lo);
  return (char)(w >> (8u * (code & 7u)) & 0xFFu);
}

// what the caller wants of pass B
struct BamTextAsk {
  bool pool = false;      // the pool's arrays (else the FASTA texts)
  bool names = false;     // pool: names too
  bool unmapped = false;  // the unmapped reads too
  // pool form on the device: the bases stay there (BamText::d_text) in the pooled build's layout, every read followed
  // by one 'N'; no bases and no names come down, pnoff does.  The host walk does not know it and makes what it always
  // makes.
  bool device_text = false;
};

// what pass B makes, on the host walk and on the device alike (the members stand in the order the two-pass route has
// always allocated and released them in)
struct BamText {
  // text form: where row r's FASTA record lies in `text` (0, 0 for a row nothing selected), the selected rows' records
  // back to back, and the unmapped reads' text with their count
  std::vector<uint64_t> toff;
  std::vector<uint32_t> tlen;
  std::string text, unmapped;
  int64_t n_unmapped = 0;
  // pool form: every held record once, in file order — its bases, its name when asked for, its index by row (0 for a
  // row that is not held), and the indices of the unmapped ones
  std::string pbases, pnames;
  std::vector<uint64_t> pboff{0}, pnoff{0};
  std::vector<uint32_t> pidx, punmapped;
  // device_text: one device allocation of d_bytes bytes, the caller's to hipFree on `d_device` — the text, and at
  // d_start the held reads' starts in it (pboff.size() entries; pboff[i] is d_start[i] - i); pbases and pnames empty
  void* d_text = nullptr;
  const uint64_t* d_start = nullptr;
  uint64_t d_bytes = 0;
  int d_device = -1;
};

// Pass B on the device of `rows`, whose resident stream and record offsets must be there; sel[r] != 0 for the rows of
// lists 1 and 2 (rows().n bytes on the host).  False: *why; nothing of *out is to be used, and the caller takes the
// host route.
bool bam_text_device(const BamRowsDevice& rows, const uint8_t* sel, const BamTextAsk& ask, BamText* out, std::string* why);

}  // namespace g2s
