// gap2seq_amd/csrc/kmer.hpp — 2-bit k-mer arithmetic with GATB-core's codec.
//
// Replaces the k-mer model behind gatb Graph::buildNode / Node::kmer used at
// /root/reference/src/Gap2Seq.cpp:879,955,995,1084,1114 (GATB-core 1.4.1 is
// un-vendored; semantics from SURVEY.md Appendix B.1-B.3):
//   code(c) = (c>>1)&3  -> A 0, C 1, T 2, G 3 (any byte maps to some base)
//   invalid(c) = (c>>3)&1 -> true for N/n, used only when counting k-mers
//   first base most significant; complement = code ^ 2
//   canonical = numeric min(forward, revcomp); strand 0 iff forward < revcomp
//   64-bit words for k <= 31, 128-bit for 32 <= k <= 63, 256-bit (u256) for 64 <= k <= 127.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define G2S_HD __host__ __device__
#else
#define G2S_HD
#endif

namespace g2s {

typedef unsigned __int128 u128;

// 256-bit unsigned integer: what the k-mer templates ask of their word type (shifts, bitwise operations, subtraction,
// numeric order, construction from small integers, truncating casts), on the host and on the device.  Two 128-bit
// halves, the low one first in memory: a k-mer array is four little-endian 64-bit words, least significant first.
// Order is numeric, most significant half first (GATB's A < C < T < G, first base most significant).
struct u256 {
  u128 lo, hi;
  G2S_HD u256() : lo(0), hi(0) {}
  G2S_HD u256(uint64_t x) : lo(x), hi(0) {}
  G2S_HD u256(u128 h, u128 l) : lo(l), hi(h) {}
  G2S_HD explicit operator uint64_t() const { return (uint64_t)lo; }
  G2S_HD explicit operator uint32_t() const { return (uint32_t)lo; }
  G2S_HD explicit operator uint8_t() const { return (uint8_t)lo; }
  G2S_HD explicit operator int() const { return (int)(uint32_t)lo; }
  G2S_HD uint64_t word(int i) const {  // 64-bit word i, 0 = least significant
    return (uint64_t)((i & 2) ? (hi >> (64 * (i & 1))) : (lo >> (64 * (i & 1))));
  }
};
static_assert(sizeof(u256) == 32, "u256 is four 64-bit words");

G2S_HD inline u256 operator<<(const u256& a, int s) {
  if (s <= 0) return a;
  if (s >= 256) return u256();
  if (s >= 128) return u256(a.lo << (s - 128), (u128)0);
  return u256((a.hi << s) | (a.lo >> (128 - s)), a.lo << s);
}
G2S_HD inline u256 operator>>(const u256& a, int s) {
  if (s <= 0) return a;
  if (s >= 256) return u256();
  if (s >= 128) return u256((u128)0, a.hi >> (s - 128));
  return u256(a.hi >> s, (a.lo >> s) | (a.hi << (128 - s)));
}
G2S_HD inline u256 operator|(const u256& a, const u256& b) { return u256(a.hi | b.hi, a.lo | b.lo); }
G2S_HD inline u256 operator&(const u256& a, const u256& b) { return u256(a.hi & b.hi, a.lo & b.lo); }
G2S_HD inline u256 operator^(const u256& a, const u256& b) { return u256(a.hi ^ b.hi, a.lo ^ b.lo); }
G2S_HD inline u256 operator~(const u256& a) { return u256(~a.hi, ~a.lo); }
G2S_HD inline u256 operator-(const u256& a, const u256& b) { return u256(a.hi - b.hi - (a.lo < b.lo ? 1 : 0), a.lo - b.lo); }
G2S_HD inline u256& operator<<=(u256& a, int s) { return a = a << s; }
G2S_HD inline u256& operator>>=(u256& a, int s) { return a = a >> s; }
G2S_HD inline bool operator==(const u256& a, const u256& b) { return a.hi == b.hi && a.lo == b.lo; }
G2S_HD inline bool operator!=(const u256& a, const u256& b) { return !(a == b); }
G2S_HD inline bool operator<(const u256& a, const u256& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

static inline int nt_code(char c) { return (c >> 1) & 3; }
static inline bool nt_invalid(char c) { return ((c >> 3) & 1) != 0; }
static const char kNtChar[4] = {'A', 'C', 'T', 'G'};

static inline uint64_t revcomp32(uint64_t x) {  // all 32 bases of a word
  x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
  x = __builtin_bswap64(x);
  return x ^ 0xAAAAAAAAAAAAAAAAULL;
}

template <class KT>
struct KmerOps;

template <>
struct KmerOps<uint64_t> {
  static uint64_t mask(int k) { return k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1); }
  static uint64_t revcomp(uint64_t x, int k) { return revcomp32(x) >> (64 - 2 * k); }
  static uint64_t hash(uint64_t z) {
    z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdULL;
    z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ULL;
    return z ^ (z >> 33);
  }
};

template <>
struct KmerOps<u128> {
  static u128 mask(int k) { return k >= 64 ? ~(u128)0 : (((u128)1 << (2 * k)) - 1); }
  static u128 revcomp(u128 x, int k) {
    u128 y = ((u128)revcomp32((uint64_t)x) << 64) | (u128)revcomp32((uint64_t)(x >> 64));
    return y >> (128 - 2 * k);
  }
  static uint64_t hash(u128 x) {
    return KmerOps<uint64_t>::hash((uint64_t)x) ^ KmerOps<uint64_t>::hash((uint64_t)(x >> 64) ^ 0x9e3779b97f4a7c15ULL);
  }
};

template <>
struct KmerOps<u256> {
  static u256 mask(int k) { return k >= 128 ? ~u256() : (~u256()) >> (256 - 2 * k); }
  static u256 revcomp(u256 x, int k) {
    const u128 h = ((u128)revcomp32(x.word(0)) << 64) | (u128)revcomp32(x.word(1));
    const u128 l = ((u128)revcomp32(x.word(2)) << 64) | (u128)revcomp32(x.word(3));
    return u256(h, l) >> (256 - 2 * k);
  }
  static uint64_t hash(u256 x) {
    return KmerOps<u128>::hash(x.lo) ^ KmerOps<u128>::hash(x.hi ^ (u128)0x85ebca6b27d4eb4fULL);
  }
};

// Rolling forward/reverse encoder over a sequence.
template <class KT>
struct KmerRoller {
  int k;
  KT mask, fwd = 0, rev = 0;
  int valid = 0;
  explicit KmerRoller(int kk) : k(kk), mask(KmerOps<KT>::mask(kk)) {}
  // returns true when a full valid k-mer ends at this character
  bool push(char c) {
    if (nt_invalid(c)) { valid = 0; fwd = 0; rev = 0; return false; }
    KT code = (KT)nt_code(c);
    fwd = ((fwd << 2) | code) & mask;
    rev = (rev >> 2) | ((code ^ 2) << (2 * (k - 1)));
    return ++valid >= k;
  }
  KT canonical() const { return fwd < rev ? fwd : rev; }
};

// buildNode: encode the first k chars regardless of validity.
template <class KT>
static inline void encode_kmer(const char* s, int k, KT* canon, int* strand) {
  KT f = 0;
  for (int i = 0; i < k; i++) f = (f << 2) | (KT)nt_code(s[i]);
  KT r = KmerOps<KT>::revcomp(f, k);
  if (f < r) { *canon = f; *strand = 0; } else { *canon = r; *strand = 1; }
}

template <class KT>
static inline std::string decode_kmer(KT canon, int strand, int k) {
  KT seq = strand == 0 ? canon : KmerOps<KT>::revcomp(canon, k);
  std::string s((size_t)k, 'A');
  for (int i = k - 1; i >= 0; i--) { s[(size_t)i] = kNtChar[(int)(seq & 3)]; seq >>= 2; }
  return s;
}

}  // namespace g2s
