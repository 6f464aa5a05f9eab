// gap2seq_amd/csrc/inflate_core.h — RFC 1951 raw deflate for ONE BGZF member (at most 64 KiB inflated), written once
// for the host (bam.cpp's test path, tools/inflate_fuzz.cpp) and for the device (bgzf_inflate.hip: one wave a member),
// and the CRC-32 arithmetic the device checks a member's trailer with (RFC 1952 section 8; slices combined by
// multiplication by x^(8 * length) modulo the polynomial, as zlib's crc32_combine does).
//
// The decoder is the same statements on both sides.  What differs is how bytes are written: the Sink.
//   sink.put(at, byte)              one literal at output offset `at`
//   sink.match(at, dist, len)       len bytes at `at`, copied from `at - dist` (dist < len: periodic with period dist)
//   sink.copy_in(at, src, len)      len bytes of a stored block
//   sink.finish()                   everything handed over is in place
// `at` only ever grows, by exactly the bytes handed over.
//
// Safe on any input: every read of compressed bytes is bounded by the member's deflate length `n` (past it the bit
// reader feeds zero bits and the decoder stops at the next check: overrun()), every write is checked against `isize`
// BEFORE the sink sees it, a distance never reaches in front of the member's first byte, and every loop either consumes
// input bits (whose number is checked against 8 n once a symbol) or is bounded by a table size.  An error is a return
// value.  What is accepted is what zlib's inflate accepts: over-subscribed codes and incomplete codes are errors, except
// — as in zlib — a literal/length or distance code with no code longer than one bit (a single one-bit code, or for
// distances none at all), whose unused code is an error when it is met; bytes behind the final block are ignored.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define G2S_INF_FN __host__ __device__ __forceinline__
#define G2S_INF_CX constexpr __host__ __device__
#else
#define G2S_INF_FN inline
#define G2S_INF_CX constexpr
#endif
// a value every lane of the wave holds alike (table entries, input words): said so, so that the decoder's state and
// its branches stay on the scalar unit
#if defined(__HIP_DEVICE_COMPILE__)
#define G2S_INF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define G2S_INF_UNIFORM(x) ((uint32_t)(x))
#endif

namespace g2s {
namespace inflate {

enum : uint32_t { kOk = 0, kCorrupt = 1, kSizeMismatch = 2, kCrcMismatch = 3 };

constexpr uint32_t kMaxMember = 65536;  // inflated bytes of a member (bam.cpp: index_blocks)
constexpr uint32_t kLitBits = 10, kDistBits = 9, kClBits = 7;  // index bits of the one-step tables
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kMaxCl = 19;

// The decode tables of the block being read.  A code is: count[l] = its symbols of length l; sym[] = its symbols by
// (length, value), the canonical order; fast[] = one step for the codes of at most `bits` bits, indexed by the next
// `bits` input bits: symbol << 4 | length, 0 = longer code (or none).  The code-length code borrows the distance
// code's count / sym and the literal table's first 128 entries.
struct Tables {
  uint16_t lit_fast[1u << kLitBits];
  uint16_t dist_fast[1u << kDistBits];
  uint16_t lit_sym[kMaxLit];
  uint16_t dist_sym[kMaxDist];
  uint16_t lit_count[16], dist_count[16], offs[16];
  uint8_t lens[kMaxLit + kMaxDist];
  uint8_t cl[kMaxCl + 1];
};

// ---- bits, least significant first
struct Bits {
  const uint8_t* in;
  uint32_t n;    // the member's deflate bytes
  uint32_t pos;  // bytes taken into `buf`, the zero bytes fed behind the end included
  uint32_t cnt;
  uint64_t buf;
  G2S_INF_FN uint32_t load32() const {
    uint32_t w = 0;
    if (pos + 4u <= n) {
      memcpy(&w, in + pos, 4);
    } else {
      for (uint32_t i = 0; i < 4u; i++)
        if (pos + i < n) w |= (uint32_t)in[pos + i] << (8u * i);
    }
    return G2S_INF_UNIFORM(w);
  }
  // at least 33 bits afterwards
  G2S_INF_FN void refill() {
    if (cnt <= 32u) {
      buf |= (uint64_t)load32() << cnt;
      cnt += 32u;
      pos += 4u;
    }
  }
  G2S_INF_FN uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }
  G2S_INF_FN void drop(uint32_t k) { buf >>= k; cnt -= k; }
  G2S_INF_FN uint32_t take(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }
  // bits were consumed that the member does not have
  G2S_INF_FN bool overrun() const { return (uint64_t)pos * 8u - cnt > (uint64_t)n * 8u; }
};

G2S_INF_FN uint32_t reverse_bits(uint32_t v, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; i++) { r = r << 1 | (v & 1u); v >>= 1; }
  return r;
}

// The canonical code of lens[0, n).  False: over-subscribed, or incomplete — unless `one_bit_ok` and no code is longer
// than one bit.
G2S_INF_FN bool build_code(const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* sym, uint16_t* offs, uint16_t* fast,
                           uint32_t fast_bits, bool one_bit_ok) {
  for (uint32_t l = 0; l < 16u; l++) count[l] = 0;
  for (uint32_t i = 0; i < n; i++) count[lens[i] & 15u]++;
  int32_t left = 1;
  uint32_t longest = 0;
  for (uint32_t l = 1; l < 16u; l++) {
    const uint32_t c = G2S_INF_UNIFORM(count[l]);
    left = left * 2 - (int32_t)c;
    if (left < 0) return false;
    if (c) longest = l;
  }
  if (left > 0 && !(one_bit_ok && longest <= 1u)) return false;
  offs[1] = 0;
  for (uint32_t l = 1; l < 15u; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lens[i] & 15u;
    if (l) sym[offs[l]++] = (uint16_t)i;
  }
  for (uint32_t i = 0; i < (1u << fast_bits); i++) fast[i] = 0;
  uint32_t code = 0, at = 0;
  for (uint32_t l = 1; l <= fast_bits; l++) {
    const uint32_t c = G2S_INF_UNIFORM(count[l]);
    for (uint32_t j = 0; j < c; j++, code++, at++) {
      const uint16_t e = (uint16_t)(sym[at] << 4 | l);
      for (uint32_t x = reverse_bits(code, l); x < (1u << fast_bits); x += 1u << l) fast[x] = e;
    }
    code <<= 1;
  }
  return true;
}

// the next symbol, or -1 when the bits are no code of this (incomplete) code
G2S_INF_FN int32_t decode_sym(Bits& b, const uint16_t* count, const uint16_t* sym, const uint16_t* fast, uint32_t fast_bits) {
  b.refill();
  const uint32_t e = G2S_INF_UNIFORM(fast[b.peek(fast_bits)]);
  if (e) { b.drop(e & 15u); return (int32_t)(e >> 4); }
  uint32_t bits = b.peek(15), code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16u; l++) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t c = G2S_INF_UNIFORM(count[l]);
    if (code < first + c) { b.drop(l); return (int32_t)G2S_INF_UNIFORM(sym[index + (code - first)]); }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// RFC 1951 3.2.5: match lengths 257..285 and distances 0..29, base value and extra bits
G2S_INF_FN uint32_t len_base(uint32_t s) {
  const uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  return t[s];
}
G2S_INF_FN uint32_t len_extra(uint32_t s) {
  const uint8_t t[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  return t[s];
}
G2S_INF_FN uint32_t dist_base(uint32_t s) {
  const uint16_t t[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  return t[s];
}
G2S_INF_FN uint32_t dist_extra(uint32_t s) {
  const uint8_t t[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  return t[s];
}
// 3.2.7: the order in which the code-length code's lengths are sent
G2S_INF_FN uint32_t cl_order(uint32_t i) {
  const uint8_t t[kMaxCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return t[i];
}

// 3.2.6: the fixed code.  Literals 286 / 287 and distances 30 / 31 have codes and are errors when met.
G2S_INF_FN bool fixed_tables(Tables* T) {
  for (uint32_t i = 0; i < kMaxLit; i++) T->lens[i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : 8);
  for (uint32_t i = 0; i < kMaxDist; i++) T->lens[kMaxLit + i] = 5;
  return build_code(T->lens, kMaxLit, T->lit_count, T->lit_sym, T->offs, T->lit_fast, kLitBits, true) &&
         build_code(T->lens + kMaxLit, kMaxDist, T->dist_count, T->dist_sym, T->offs, T->dist_fast, kDistBits, true);
}

// 3.2.7: the dynamic header.  The repeat codes 16 / 17 / 18 run over the literal/length and distance lengths as one list.
G2S_INF_FN bool dynamic_tables(Bits& b, Tables* T) {
  b.refill();
  const uint32_t hlit = b.take(5) + 257u, hdist = b.take(5) + 1u, hclen = b.take(4) + 4u;
  if (hlit > 286u || hdist > 30u) return false;
  for (uint32_t i = 0; i < kMaxCl; i++) T->cl[i] = 0;
  for (uint32_t i = 0; i < hclen; i++) {
    if ((i & 7u) == 0) b.refill();
    T->cl[cl_order(i)] = (uint8_t)b.take(3);
  }
  if (!build_code(T->cl, kMaxCl, T->dist_count, T->dist_sym, T->offs, T->lit_fast, kClBits, false)) return false;
  const uint32_t total = hlit + hdist;
  uint32_t at = 0;
  while (at < total) {
    if (b.overrun()) return false;
    const int32_t s = decode_sym(b, T->dist_count, T->dist_sym, T->lit_fast, kClBits);
    if (s < 0) return false;
    if (s < 16) { T->lens[at++] = (uint8_t)s; continue; }
    uint32_t prev = 0, rep;
    if (s == 16) {
      if (at == 0) return false;
      prev = G2S_INF_UNIFORM(T->lens[at - 1]);
      rep = 3u + b.take(2);
    } else if (s == 17) {
      rep = 3u + b.take(3);
    } else {
      rep = 11u + b.take(7);
    }
    if (at + rep > total) return false;
    for (; rep; rep--) T->lens[at++] = (uint8_t)prev;
  }
  if (G2S_INF_UNIFORM(T->lens[256]) == 0) return false;  // (no end-of-block code)
  return build_code(T->lens, hlit, T->lit_count, T->lit_sym, T->offs, T->lit_fast, kLitBits, true) &&
         build_code(T->lens + hlit, hdist, T->dist_count, T->dist_sym, T->offs, T->dist_fast, kDistBits, true);
}

// One member: `n` deflate bytes at `in`, `isize` bytes out through the sink.  kOk, kCorrupt or kSizeMismatch.
template <class Sink>
G2S_INF_FN uint32_t inflate_member(const uint8_t* in, uint32_t n, uint32_t isize, Tables* T, Sink& sink) {
  Bits b{in, n, 0, 0, 0};
  uint32_t out_n = 0;
  for (;;) {
    b.refill();
    const uint32_t last = b.take(1), type = b.take(2);
    if (type == 3u) return kCorrupt;
    if (type == 0u) {
      b.drop(b.cnt & 7u);
      b.refill();
      const uint32_t len = b.take(16), nlen = b.take(16);
      if (len != (~nlen & 0xFFFFu) || b.overrun()) return kCorrupt;
      const uint32_t from = b.pos - b.cnt / 8u;  // (cnt is a multiple of 8 here, and from <= n: no overrun)
      if (len > n - from) return kCorrupt;
      if (len > isize - out_n) return kSizeMismatch;
      if (len) sink.copy_in(out_n, in + from, len);
      out_n += len;
      b.pos = from + len;
      b.cnt = 0;
      b.buf = 0;
    } else {
      if (!(type == 1u ? fixed_tables(T) : dynamic_tables(b, T))) return kCorrupt;
      for (;;) {
        if (b.overrun()) return kCorrupt;
        int32_t s = decode_sym(b, T->lit_count, T->lit_sym, T->lit_fast, kLitBits);
        if (s < 0) return kCorrupt;
        if (s < 256) {
          if (out_n >= isize) return kSizeMismatch;
          sink.put(out_n++, (uint8_t)s);
          continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) return kCorrupt;  // (286, 287)
        const uint32_t len = len_base((uint32_t)s) + b.take(len_extra((uint32_t)s));
        const int32_t d = decode_sym(b, T->dist_count, T->dist_sym, T->dist_fast, kDistBits);
        if (d < 0 || d >= 30) return kCorrupt;
        const uint32_t dist = dist_base((uint32_t)d) + b.take(dist_extra((uint32_t)d));
        if (dist > out_n) return kCorrupt;
        if (len > isize - out_n) return kSizeMismatch;
        sink.match(out_n, dist, len);
        out_n += len;
      }
    }
    if (b.overrun()) return kCorrupt;
    if (last) break;
  }
  sink.finish();
  return out_n == isize ? kOk : kSizeMismatch;
}

// the host's sink: plain stores
struct HostSink {
  uint8_t* out;
  void put(uint32_t at, uint8_t c) { out[at] = c; }
  void match(uint32_t at, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[at + i] = out[at + i - dist];
  }
  void copy_in(uint32_t at, const uint8_t* src, uint32_t len) { memcpy(out + at, src, len); }
  void finish() {}
};

// ---- CRC-32 (reflected, polynomial 0xEDB88320)
constexpr uint32_t kCrcPoly = 0xEDB88320u;

G2S_INF_CX uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
// a(x) b(x) mod P; bit 31 is x^0
G2S_INF_CX uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
struct CrcPowers { uint32_t v[32]; };  // x^(2^i)
G2S_INF_CX CrcPowers crc_powers() {
  CrcPowers t{};
  uint32_t p = 1u << 30;  // x^1
  for (int i = 0; i < 32; i++) { t.v[i] = p; p = crc_mul(p, p); }
  return t;
}
// x^(8 * bytes) mod P
G2S_INF_FN uint32_t crc_x8n(uint32_t bytes) {
  constexpr CrcPowers t = crc_powers();
  uint32_t p = 1u << 31;  // x^0
  for (uint32_t k = 3; bytes; bytes >>= 1, k++)
    if (bytes & 1u) p = crc_mul(t.v[k & 31u], p);
  return p;
}
// the same for a length of 64 bits (gzip_chunks.h: a gzip member may hold more than 4 GiB), the power squared as the
// length's bits go by
G2S_INF_FN uint32_t crc_x8n64(uint64_t bytes) {
  constexpr CrcPowers t = crc_powers();
  uint32_t p = 1u << 31, sq = t.v[3];  // x^0, x^8
  for (; bytes; bytes >>= 1) {
    if (bytes & 1u) p = crc_mul(sq, p);
    sq = crc_mul(sq, sq);
  }
  return p;
}
G2S_INF_FN uint32_t crc_shift64(uint32_t crc, uint64_t bytes_behind) { return crc_mul(crc_x8n64(bytes_behind), crc); }
// the running (not yet inverted) CRC over one more byte
G2S_INF_FN uint32_t crc_byte(const uint32_t* table, uint32_t c, uint8_t v) { return table[(c ^ v) & 0xFFu] ^ (c >> 8); }
// CRC(A || B) = crc_shift(CRC(A), |B|) ^ CRC(B), for finished CRCs; an empty piece has CRC 0
G2S_INF_FN uint32_t crc_shift(uint32_t crc, uint32_t bytes_behind) { return crc_mul(crc_x8n(bytes_behind), crc); }

// The slices the device cuts a member into: lane i takes [i * slice, (i + 1) * slice) clipped to isize.  A whole
// number of words, and an odd one, so that the 64 lanes' reads fall into different LDS banks.
G2S_INF_FN uint32_t crc_slice_bytes(uint32_t isize) {
  const uint32_t words = (isize + 255u) / 256u;
  return 4u * (words | 1u);
}

// the member's CRC-32 the way the kernel computes it, its 64 lanes one after another (host: tests)
inline uint32_t crc_by_slices(const uint8_t* p, uint32_t isize) {
  uint32_t table[256];
  for (uint32_t i = 0; i < 256u; i++) table[i] = crc_table_entry(i);
  const uint32_t slice = crc_slice_bytes(isize);
  uint32_t x = 0;
  for (uint32_t lane = 0; lane < 64u; lane++) {
    const uint32_t lo = lane * slice < isize ? lane * slice : isize;
    const uint32_t hi = lo + slice < isize ? lo + slice : isize;
    if (hi == lo) continue;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t o = lo; o < hi; o++) c = crc_byte(table, c, p[o]);
    x ^= crc_shift(~c, isize - hi);
  }
  return x;
}

}  // namespace inflate
}  // namespace g2s
