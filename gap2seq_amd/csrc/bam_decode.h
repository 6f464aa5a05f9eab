// gap2seq_amd/csrc/bam_decode.h — one BAM record's output bytes made by the lanes of a wave, for the kernels that decode
// records from a resident inflated stream: pass B of the read filter (bam_text.hip: k_decode) and the graph build's text
// (bam_reads.hip: k_bamreads_write).  Device code only; the base's character is bam_text.h's base_char.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bam.hpp"
#include "bam_text.h"

namespace g2s {
namespace bam_decode {

constexpr uint32_t kWave = 64;
constexpr uint32_t kRecHead = 36;  // block_size and the 32 fixed bytes

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// kBases: the read as sequenced (a reverse-strand record from its end, complemented), 'N' behind its last base
// kName:  name / end          kFasta:  > name / end \n bases \n
enum Piece : int { kBases = 0, kName = 1, kFasta = 2 };

// `len` bytes of one record's output at dst, by the lanes of a wave: byte i by lane i mod 64
template <int PIECE>
__device__ __forceinline__ void emit(const uint8_t* __restrict__ rec, uint64_t len, uint8_t* __restrict__ dst, uint32_t lane) {
  const uint32_t l_name = rec[12], w = ld32(rec + 16), n_cigar = w & 0xFFFFu, flag = w >> 16;
  const uint64_t l_seq = ld32(rec + 20);
  const uint8_t* name = rec + kRecHead;
  const uint8_t* seq = name + l_name + 4u * (size_t)n_cigar;
  const bool reverse = (flag & g2s::BAM_REVERSE) != 0;
  const char end = (flag & g2s::BAM_READ1) ? '1' : '2';
  // the name's length follows from the piece's: nothing is searched twice
  const uint64_t nl = PIECE == kName ? len - 2 : PIECE == kFasta ? len - 5 - l_seq : 0;
  auto base = [&](uint64_t j) {
    const uint64_t at = reverse ? l_seq - 1 - j : j;
    return g2s::base_char((uint32_t)(seq[at >> 1] >> ((~at & 1u) << 2)) & 15u, reverse);
  };
  for (uint64_t i = lane; i < len; i += kWave) {
    char c;
    if (PIECE == kBases) {
      c = i < l_seq ? base(i) : 'N';
    } else if (PIECE == kName) {
      c = i < nl ? (char)name[i] : i == nl ? '/' : end;
    } else {  // > name /1 \n bases \n
      if (i == 0) c = '>';
      else if (i <= nl) c = (char)name[i - 1];
      else if (i == nl + 1) c = '/';
      else if (i == nl + 2) c = end;
      else if (i == nl + 3) c = '\n';
      else if (i - (nl + 4) < l_seq) c = base(i - (nl + 4));
      else c = '\n';
    }
    dst[i] = (uint8_t)c;
  }
}

}  // namespace bam_decode
}  // namespace g2s
