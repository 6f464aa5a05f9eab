// gap2seq_amd/csrc/seg_tables.h — see seg_tables.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define G2S_REM_CAP 65535u /* rem[] saturates here: longer unitigs are walked in several segments */

namespace g2s {

// rem[v] for every oriented node (2n entries), from the device copy of the unitig-start bitmap.
hipError_t build_rem_table(const uint64_t* ustart_dev, uint64_t n, uint32_t** rem_out);
// urec[v] (8 words per oriented node) = {succ[last node of v's unitig walk][0..3], rem[v], 0, 0, 0}
hipError_t build_urec_table(const uint32_t* succ_dev, const uint32_t* rem_dev, uint64_t n, uint32_t** urec_out);
// Graphs with an explicit predecessor table (even k): brec[x], urec's layout, for the BACKWARD walks of phase A.  The walk
// back from the oriented node v covers the k-mer indices the forward walk from x = v ^ 1 covers, and ends at the node b that
// spells the reverse complement of that walk's last node e: b = e ^ 1, or e itself where e ^ 1 is the strand of a palindrome
// that does not exist.  brec[x] = {pred[b][q] ^ 1 (INVALID stays INVALID), q = 0..3, rem[x], 0, 0, 0}: a kernel that reads
// the record at v ^ 1 and flips its words, as it does with urec at odd k, holds b's true predecessors — a palindrome among
// them under the id that exists, and a palindrome's own at the index of its other strand.
hipError_t build_brec_table(const uint32_t* succ_dev, const uint32_t* pred_dev, const uint32_t* rem_dev, uint64_t n,
                            uint32_t** brec_out);

}  // namespace g2s
