// gap2seq_amd/csrc/device_pool.h — g2s_device_pool (include/g2s.h): a read pool whose bases stay where pass B of the
// read filter made them.  Device-held: one device allocation with the pool's text in the pooled build's layout (every
// read followed by one 'N') and, behind it, the reads' starts in it as 64-bit offsets (n_reads + 1 entries: read r lies
// at start[r] = base_off[r] + r, base_off[r + 1] - base_off[r] characters long).  Host-held: the same text in host
// memory.  The view's arrays are the handle's either way; its bases and names are NULL (names are never kept: the
// callers want their lengths alone).  Made by readfilter_gaps.cpp, read by api_graph.hip (g2s_graph_build_dpool_reach).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/g2s.h"

struct g2s_device_pool {
  g2s_read_pool view{};
  std::vector<uint64_t> base_off{0}, name_off{0}, gap_begin{0};
  std::vector<uint32_t> gap_read, unmapped_read;
  int device = -1;              // the device of d_text, -1: host_text
  void* d_text = nullptr;       // the allocation: text, then (256-byte aligned) the starts
  const uint64_t* d_start = nullptr;
  uint64_t device_bytes = 0;
  std::string host_text;        // host-held: every read followed by 'N'
  uint64_t text_bytes() const { return base_off.back() + (uint64_t)(base_off.size() - 1); }
  uint64_t start(uint64_t r) const { return base_off[(size_t)r] + r; }
};

namespace g2s {

// bam_text.hip: the two things a handle does with its device allocation
void device_pool_release(int device, void* p);
bool device_pool_copy_down(int device, const void* d_text, uint64_t off, uint64_t n, void* dst, std::string* why);

// g2s_test_last_dpool's filter half: the process's last g2s_filter_reads_gaps_dpool[_mem]
struct LastDpoolFilter {
  int held_on_device = 0;
  uint64_t bases_bytes_to_host = 0;
};
LastDpoolFilter last_dpool_filter();

}  // namespace g2s
