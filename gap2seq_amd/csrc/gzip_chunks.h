// gap2seq_amd/csrc/gzip_chunks.h — one deflate stream decoded from many places at once (the scheme of pugz and
// rapidgzip), written once for the host (g2s_test_gzip_inflate's device -2, tools/inflate_fuzz.cpp) and for the device
// (gzip_inflate.hip).  It stands on inflate_core.h: its bit reader, its tables, its CRC arithmetic.
//
// The deflate bytes of a window are cut into chunks of equal size.  Four steps:
//   find     for chunk c >= 1 the first bit offset inside the chunk at which a non-final dynamic block can begin:
//            accept_start() — BFINAL = 0, BTYPE = 2, and the header passes dynamic_tables(): all three codes complete by
//            zlib's rule, an end-of-block code present.  A chunk without one is absorbed by the chunk in front of it.
//            prefilter() is the part of the test one lane can do alone (the three bits, HLIT / HDIST, the code-length
//            code's Kraft sum); what passes it is handed to accept_start().
//   decode   decode_chunk() from a start to the next found start, writing 16-bit symbols: 0 .. 255 a literal,
//            256 + j "byte j of the 32 768 bytes in front of this chunk's first output byte" (a marker).  It ends in one
//            of the five states below.
//   chain    chain_byte(): the resolved last 32 768 bytes behind chunk c from chunk c's symbols and the window behind
//            chunk c - 1; a chunk that produced fewer keeps the tail of the older window in front of its own bytes.
//   resolve  resolve_sym(): a literal as it is, a marker from the window in front of its chunk.
//
// Safe on any input, as inflate_core.h: every read of compressed bytes is bounded by the window's n bytes (behind them
// the bit reader feeds zeros and the next check ends the chunk), every write is checked against the slot's capacity
// BEFORE the sink sees it, and every loop consumes input bits or is bounded by a table.  Garbage decoded from a false
// start ends in a status.
//
// The Sink of decode_chunk():
//   sink.put(at, sym)               one literal at output offset `at` of the chunk
//   sink.match(at, dist, len)       len symbols at `at`, copied from `at - dist`; a source in front of the chunk's first
//                                   symbol is the marker marker_of(at - dist + i)
//   sink.copy_in(at, src, len)      len bytes of a stored block
//   sink.finish()                   everything handed over is in place
#pragma once
#include "inflate_core.h"

namespace g2s {
namespace gzchunks {

namespace inf = g2s::inflate;

// how a chunk's decoder ended
enum : uint32_t {
  kEndOk = 0,        // at a block boundary that is exactly the next start
  kEndMismatch = 1,  // ran past the next start without a boundary there
  kEndFinal = 2,     // met the final block: end_bit is the bit behind it
  kEndSlotFull = 3,  // its output slot is full
  kEndCorrupt = 4,
};

constexpr uint32_t kWindow = 32768;  // deflate's history
constexpr uint64_t kNoBit = ~(uint64_t)0;

struct ChunkEnd {
  uint32_t status, out_n;
  uint64_t end_bit;
};

// the bit reader at bit offset `bit` of in[0, n); bit / 8 < n
G2S_INF_FN inf::Bits bits_at(const uint8_t* in, uint32_t n, uint64_t bit) {
  const uint32_t byte = (uint32_t)(bit >> 3);
  inf::Bits b{in + byte, n - byte, 0, 0, 0};
  b.refill();
  b.drop((uint32_t)bit & 7u);
  return b;
}
// where it stands, as a bit offset of `in`
G2S_INF_FN uint64_t bit_of(const inf::Bits& b, const uint8_t* in) {
  return ((uint64_t)(b.in - in) + b.pos) * 8u - b.cnt;
}

// k <= 25 bits at bit offset `bit`; bytes behind n read as zero
G2S_INF_FN uint32_t peek_bits(const uint8_t* in, uint32_t n, uint64_t bit, uint32_t k) {
  const uint64_t byte = bit >> 3;
  uint32_t w = 0;
  for (uint32_t i = 0; i < 4u; i++)
    if (byte + i < n) w |= (uint32_t)in[byte + i] << (8u * i);
  return (w >> ((uint32_t)bit & 7u)) & ((1u << k) - 1u);
}

// What one lane can tell alone of accept_start(): necessary, not sufficient.
G2S_INF_FN bool prefilter(const uint8_t* in, uint32_t n, uint64_t bit) {
  const uint32_t h = peek_bits(in, n, bit, 17);
  if ((h & 7u) != 4u) return false;  // BFINAL 0, BTYPE 2 (least significant bit first)
  if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
  const uint32_t hclen = ((h >> 13) & 15u) + 4u;
  uint32_t sum = 0;  // the code-length code's Kraft sum in units of 2^-7: complete is 128 (build_code, one_bit_ok false)
  uint64_t p = bit + 17u;
  for (uint32_t i = 0; i < hclen; i += 8u, p += 24u) {
    uint32_t w = peek_bits(in, n, p, 24);
    const uint32_t cnt = hclen - i < 8u ? hclen - i : 8u;
    for (uint32_t j = 0; j < cnt; j++, w >>= 3) {
      const uint32_t l = w & 7u;
      if (l) sum += 128u >> l;
    }
  }
  return sum == 128u;
}

// The acceptance test of a block start.  Wave-uniform on the device: every lane runs it on the same `bit`.
G2S_INF_FN bool accept_start(const uint8_t* in, uint32_t n, uint64_t bit, inf::Tables* T) {
  if ((bit >> 3) >= n) return false;
  inf::Bits b = bits_at(in, n, bit);
  if (b.take(3) != 4u) return false;
  if (!inf::dynamic_tables(b, T)) return false;
  return !b.overrun();
}

// the first accepted bit offset in [lo, hi), one offset after another (the host's finder)
inline uint64_t find_start(const uint8_t* in, uint32_t n, uint64_t lo, uint64_t hi, inf::Tables* T) {
  for (uint64_t bit = lo; bit < hi; bit++)
    if (prefilter(in, n, bit) && accept_start(in, n, bit, T)) return bit;
  return kNoBit;
}

// the marker for the chunk-relative source position s < 0 (s >= -32768: a distance is at most 32 768)
G2S_INF_FN uint16_t marker_of(int64_t s) { return (uint16_t)(256 + (int64_t)kWindow + s); }

// One chunk: from bit `start` of in[0, n) up to the block boundary `stop` (kNoBit: up to the final block), at most
// `cap` symbols through the sink.  first: the chunk has no history (a member's first), a distance beyond the symbols
// produced is then an error, as in inflate_member.
template <class Sink>
G2S_INF_FN ChunkEnd decode_chunk(const uint8_t* in, uint32_t n, uint64_t start, uint64_t stop, bool first, uint32_t cap,
                                 inf::Tables* T, Sink& sink) {
  ChunkEnd r{kEndCorrupt, 0, start};
  if ((start >> 3) >= n) return r;
  inf::Bits b = bits_at(in, n, start);
  uint32_t out_n = 0, st = kEndCorrupt;
  bool open = true;
  while (open) {
    const uint64_t here = bit_of(b, in);
    if (here >= stop) { st = here == stop ? kEndOk : kEndMismatch; break; }
    b.refill();
    const uint32_t last = b.take(1), type = b.take(2);
    if (type == 3u) break;
    if (type == 0u) {
      b.drop(b.cnt & 7u);
      b.refill();
      const uint32_t len = b.take(16), nlen = b.take(16);
      if (len != (~nlen & 0xFFFFu) || b.overrun()) break;
      const uint32_t from = b.pos - b.cnt / 8u;  // (cnt is a multiple of 8 here, and from <= b.n: no overrun)
      if (len > b.n - from) break;
      if (len > cap - out_n) { st = kEndSlotFull; break; }
      if (len) sink.copy_in(out_n, b.in + from, len);
      out_n += len;
      b.pos = from + len;
      b.cnt = 0;
      b.buf = 0;
    } else {
      if (!(type == 1u ? inf::fixed_tables(T) : inf::dynamic_tables(b, T))) break;
      for (;;) {
        if (b.overrun()) { open = false; break; }
        if (bit_of(b, in) > stop) { st = kEndMismatch; open = false; break; }  // (inside a block, behind the next start)
        int32_t s = inf::decode_sym(b, T->lit_count, T->lit_sym, T->lit_fast, inf::kLitBits);
        if (s < 0) { open = false; break; }
        if (s < 256) {
          if (out_n >= cap) { st = kEndSlotFull; open = false; break; }
          sink.put(out_n++, (uint16_t)s);
          continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) { open = false; break; }  // (286, 287)
        const uint32_t len = inf::len_base((uint32_t)s) + b.take(inf::len_extra((uint32_t)s));
        const int32_t d = inf::decode_sym(b, T->dist_count, T->dist_sym, T->dist_fast, inf::kDistBits);
        if (d < 0 || d >= 30) { open = false; break; }
        const uint32_t dist = inf::dist_base((uint32_t)d) + b.take(inf::dist_extra((uint32_t)d));
        if (first && dist > out_n) { open = false; break; }
        if (len > cap - out_n) { st = kEndSlotFull; open = false; break; }
        sink.match(out_n, dist, len);
        out_n += len;
      }
      if (!open) break;
    }
    if (b.overrun()) break;
    if (last) { st = kEndFinal; break; }
  }
  sink.finish();
  r.status = st;
  r.out_n = out_n;
  r.end_bit = bit_of(b, in);
  return r;
}

// the host's sink: plain stores into the chunk's slot
struct HostSymSink {
  uint16_t* slot;
  void put(uint32_t at, uint16_t c) { slot[at] = c; }
  void match(uint32_t at, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) {
      const int64_t s = (int64_t)at + i - dist;
      slot[at + i] = s < 0 ? marker_of(s) : slot[s];
    }
  }
  void copy_in(uint32_t at, const uint8_t* src, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) slot[at + i] = src[i];
  }
  void finish() {}
};

// a symbol's byte, `hist` the 32 768 bytes in front of its chunk
G2S_INF_FN uint8_t resolve_sym(uint16_t s, const uint8_t* hist) { return s < 256u ? (uint8_t)s : hist[(s - 256u) & (kWindow - 1u)]; }
// whether a symbol may be resolved: `valid` of the 32 768 bytes in front of its chunk exist (a member's first bytes have
// fewer in front of them; a marker that points in front of the member is a corrupt stream)
G2S_INF_FN bool sym_ok(uint16_t s, uint32_t valid) { return s < 256u || (s - 256u < kWindow && s - 256u >= kWindow - valid); }

// byte j of the window behind a chunk of out_n symbols at `slot`, `prev` the window in front of it
G2S_INF_FN uint8_t chain_byte(const uint8_t* prev, const uint16_t* slot, uint32_t out_n, uint32_t j) {
  if (out_n >= kWindow) return resolve_sym(slot[out_n - kWindow + j], prev);
  const uint32_t keep = kWindow - out_n;
  return j < keep ? prev[j + out_n] : resolve_sym(slot[j - keep], prev);
}

}  // namespace gzchunks
}  // namespace g2s
