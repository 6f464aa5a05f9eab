// gap2seq_amd/csrc/name_hash.h — the hash of a read's name with its end ("name/1", "name/2") as the batched read filter
// takes it (readfilter_gaps.cpp: pass A), written once for the host and for the device (bam_rows.hip).
//
// The filter's bits are `std::hash<std::string> % bits` of the reference's build (readfilter.cpp: NameFilter), so the
// function here is the one libstdc++ gives for std::hash<std::string> on a 64-bit target: _Hash_bytes (a variant of
// MurmurHash64A: eight bytes a step, little-endian, the tail's bytes as unsigned values) with the seed 0xc70f6907.  It
// belongs to the host library and not to this project, so nothing relies on it unchecked: before the device path's
// first use in a process the host compilation of this header is compared with std::hash<std::string> on a fixed probe
// set (readfilter_gaps.cpp: name_hash_usable), and a difference keeps pass A's rows on the host for the process.
//
// The bytes hashed are name[0 .. n) followed by '/' and the digit of `which` (1 or 2); n is strnlen(name, l_name), the
// caller's to compute.  No string is formed.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define G2S_NH_FN __host__ __device__ __forceinline__
#else
#define G2S_NH_FN inline
#endif

namespace g2s {

G2S_NH_FN uint64_t name_hash_mix(uint64_t v) { return v ^ (v >> 47); }

// byte i of the hashed text
G2S_NH_FN uint64_t name_hash_byte(const uint8_t* name, uint32_t n, uint32_t which, uint32_t i) {
  return i < n ? (uint64_t)name[i] : i == n ? (uint64_t)'/' : (uint64_t)('0' + which);
}

G2S_NH_FN uint64_t name_hash(const uint8_t* name, uint32_t n, uint32_t which) {
  const uint64_t mul = 0xc6a4a7935bd1e995ull, seed = 0xc70f6907ull;
  const uint32_t len = n + 2u, aligned = len & ~7u;
  uint64_t h = seed ^ ((uint64_t)len * mul);
  for (uint32_t o = 0; o < aligned; o += 8u) {
    uint64_t d = 0;
    for (uint32_t k = 0; k < 8u; k++) d |= name_hash_byte(name, n, which, o + k) << (8u * k);
    h ^= name_hash_mix(d * mul) * mul;
    h *= mul;
  }
  if (len & 7u) {
    uint64_t d = 0;
    for (uint32_t k = 0; k < (len & 7u); k++) d |= name_hash_byte(name, n, which, aligned + k) << (8u * k);
    h ^= d;
    h *= mul;
  }
  h = name_hash_mix(h) * mul;
  return name_hash_mix(h);
}

}  // namespace g2s
