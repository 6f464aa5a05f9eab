// gap2seq_amd/csrc/readfilter_gaps.hpp — what the per-gap read filter (readfilter.cpp) and the batched one
// (readfilter_gaps.cpp, g2s_filter_reads_gaps) share: read names, FASTA records, htslib's region semantics; and the
// joins of the batched filter, on host threads (readfilter_gaps.cpp) and on the device (readfilter_gpu.hip).
//
// The joins work on one compact row per BAM record (FilterRows, pass A) and never see a name: a name enters as its
// 64-bit std::hash, computed on the host with the compiler's own std::hash, and every comparison is between bits
// `hash % bits` of the reference's one-bit-per-name filter (readfilter.cpp: NameFilter).  Collisions modulo `bits`
// are therefore reproduced exactly.
//
// Limits (both paths): rows are indexed in 32 bits (fewer than 2^32 - 1 records a file), gaps in 29 bits (a (bit, gap)
// pair is one 64-bit key, bit << 29 | gap, and bit < 5 * 2^32 < 2^35), and the pairs a call emits — the (bit, gap)
// pairs of every gap's mate filter before de-duplication, plus both lists' (gap, row) pairs — are at most
// `max_pairs` (default 2^31, G2S_FILTER_MAX_PAIRS), else the call fails with G2S_ERR_NOMEM.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bam.hpp"
#include "bam_rows.h"

namespace g2s {

// ReadFilter.cpp:165-173: the read's name with its end, and its mate's
inline std::string own_name(const BamRec& r) {
  return std::string(r.name, strnlen(r.name, r.l_name)) + ((r.flag & BAM_READ1) ? "/1" : "/2");
}
inline std::string mate_name(const BamRec& r) {
  return std::string(r.name, strnlen(r.name, r.l_name)) + ((r.flag & BAM_READ1) ? "/2" : "/1");
}

// ReadFilter.cpp:105-161: the read as sequenced (reverse strand alignments are complemented back); every code
// other than A, C, G, T becomes N
inline void append_bases(const BamRec& r, std::string* out) {
  static const char fwd[16] = {'N', 'A', 'C', 'N', 'G', 'N', 'N', 'N', 'T', 'N', 'N', 'N', 'N', 'N', 'N', 'N'};
  static const char rev[16] = {'N', 'T', 'G', 'N', 'C', 'N', 'N', 'N', 'A', 'N', 'N', 'N', 'N', 'N', 'N', 'N'};
  const size_t at = out->size();
  out->resize(at + (size_t)r.l_seq);
  char* d = &(*out)[at];
  if (!(r.flag & BAM_REVERSE))
    for (int32_t i = 0; i < r.l_seq; i++) d[i] = fwd[r.base4(i)];
  else
    for (int32_t i = 0; i < r.l_seq; i++) d[i] = rev[r.base4(r.l_seq - 1 - i)];
}
inline void append_fasta(const BamRec& r, std::string* out) {
  out->push_back('>');
  out->append(own_name(r));
  out->push_back('\n');
  append_bases(r, out);
  out->push_back('\n');
}

// htslib's region iterator as the reference calls it (sam_itr_queryi, ReadFilter.cpp:184-191): a negative
// start is 0; an end in front of the start gives NO iterator (the reference then prints a warning and reads
// nothing, :188-190,213-217) — which is what happens to its right-hand window, whose bounds are written
// the wrong way round (:388-389), whenever the standard deviation is not 0.
struct Region {
  int tid;
  int64_t beg, end;
  bool valid;
};
inline Region make_region(int tid, int64_t beg, int64_t end, std::string* warn) {
  Region q{tid, beg < 0 ? 0 : beg, end, true};
  if (tid < 0 || q.end < q.beg) {
    q.valid = false;
    warn->append("WARNING: SAM iterator is NULL!\n");
  }
  return q;
}
// (an empty region [x, x) yields nothing and no warning: htslib's reg2bins returns no bin for beg >= end, so the
// iterator exists and ends at once — it is not a point query)
inline bool in_region(int64_t pos, int64_t end, const Region& q) { return q.valid && q.beg < q.end && pos < q.end && end > q.beg; }
inline bool overlaps(const BamRec& r, const Region& q) {
  return q.valid && q.beg < q.end && r.ref_id == q.tid && (int64_t)r.pos < q.end && r.end_pos() > q.beg;
}

// g2s_filter_last_error's text (readfilter.cpp)
void set_filter_error(const std::string& e);

// ---- the joins of the batched filter

constexpr int kFilterGapBits = 29;
constexpr uint64_t kFilterGapMask = ((uint64_t)1 << kFilterGapBits) - 1;

// pass A: one row per record, in file order
struct FilterRows {
  std::vector<int32_t> ref_id, pos;
  std::vector<int64_t> end;            // htslib's bam_endpos
  std::vector<uint32_t> flag;
  std::vector<uint64_t> h_own, h_mate; // std::hash of own_name / mate_name
  int64_t max_span = 1;                // longest end - pos of a record with ref_id >= 0
  size_t size() const { return pos.size(); }
};

// a window as the joins see it: records with ref_id == tid, pos < end and end position > beg; nothing matches when
// tid < 0 or beg >= end (an invalid or empty Region)
struct FilterWindow {
  int32_t tid, pad;
  int64_t beg, end;
};
inline FilterWindow filter_window(const Region& q) {
  FilterWindow w{-1, 0, 0, 0};
  if (q.valid && q.beg < q.end) { w.tid = q.tid; w.beg = q.beg; w.end = q.end; }
  return w;
}

// the key of the (ref_id, pos) index; ref_id -1 sorts last.  index_key(tid, p) for p in [INT32_MIN, INT32_MAX + 1]
// bounds the keys of tid's records at positions < p.
inline uint64_t filter_index_key(int32_t tid, int64_t p) {
  p = p < (int64_t)INT32_MIN ? (int64_t)INT32_MIN : p > (int64_t)INT32_MAX + 1 ? (int64_t)INT32_MAX + 1 : p;
  return ((uint64_t)(uint32_t)tid << 32) + (uint64_t)(p - (int64_t)INT32_MIN);
}

struct FilterJoin {
  // in
  const FilterRows* rows = nullptr;
  const DeviceRows* device_rows = nullptr;  // filter_join_device: the rows lie on its device already (`rows` is unused)
  uint64_t bits = 0;                   // 5 * records
  std::vector<FilterWindow> win;       // 3 a gap: left, right, around
  uint64_t max_pairs = 0;
  size_t gaps() const { return win.size() / 3; }
  // out: (gap << 32 | row), ascending — list 1 (mates of the filtered names) and list 2 (flank reads not in the filter)
  std::vector<uint64_t> list1, list2;
};

// G2S_OK, G2S_ERR_NOMEM (the pair cap, or memory), G2S_ERR_HIP (device path)
int filter_join_host(FilterJoin& j, int threads, std::string* err);
bool filter_device_usable(int device);
int filter_join_device(FilterJoin& j, int device, std::string* err);

}  // namespace g2s
