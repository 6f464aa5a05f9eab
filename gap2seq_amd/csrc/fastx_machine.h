// gap2seq_amd/csrc/fastx_machine.h — parse_fastx (fastx.cpp) as a state machine over lines, in a form that compiles for
// the host and for the device: the kernels of reads_text.hip and the host restatement the tests compare them with share
// this one definition.  No other project header, no HIP call.
//
// A line ends at '\n' (or at the end of the file); one trailing '\r' is dropped; its class is taken afterwards:
//   E empty, G first byte '>', A first byte '@', O anything else.
// parse_fastx keeps (cur != nullptr, fastq_line); as states:
//   NONE    no record open                       FA_H / FA_S  a FASTA record is open
//   Q_SEQ   a FASTQ header was read (line 0)     Q_PLUS / Q_QUAL  its lines 1 and 2
// FASTA is two states here, by whether the LAST line was sequence: the state behind a line then says by itself whether
// that line's bytes belong to the build's text (FA_S and Q_PLUS: "the line before me was sequence"), so a byte deep
// inside a line of any length needs nothing but the scanned state of its line's head.
//
//   state    E        G            A            O
//   NONE     NONE     FA_H, new    Q_SEQ, new   NONE
//   FA_H/S   FA_H     FA_H, new    FA_S         FA_S
//   Q_SEQ    Q_PLUS   (every class: the line is the sequence, even when empty)
//   Q_PLUS   Q_QUAL   (every class)
//   Q_QUAL   NONE     (every class)
//
// A transition is a function on six states, three bits a state: 18 bits of a uint32_t.  Composition is associative, so
// the state in front of every line is a scan of the lines' functions.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define G2S_FX_HD __host__ __device__ __forceinline__
#else
#define G2S_FX_HD inline
#endif

namespace g2s {
namespace fastx {

enum State : uint32_t { NONE = 0, FA_H = 1, FA_S = 2, Q_SEQ = 3, Q_PLUS = 4, Q_QUAL = 5, kStates = 6 };
enum Class : uint32_t { E = 0, G = 1, A = 2, O = 3 };

constexpr uint32_t pack6(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t s4, uint32_t s5) {
  return s0 | s1 << 3 | s2 << 6 | s3 << 9 | s4 << 12 | s5 << 15;
}
// the function that changes nothing (a byte that is no line head)
constexpr uint32_t kIdentity = pack6(NONE, FA_H, FA_S, Q_SEQ, Q_PLUS, Q_QUAL);

// the transition function of a line of class c
G2S_FX_HD uint32_t line_fn(uint32_t c) {
  constexpr uint32_t fE = pack6(NONE, FA_H, FA_H, Q_PLUS, Q_QUAL, NONE);
  constexpr uint32_t fG = pack6(FA_H, FA_H, FA_H, Q_PLUS, Q_QUAL, NONE);
  constexpr uint32_t fA = pack6(Q_SEQ, FA_S, FA_S, Q_PLUS, Q_QUAL, NONE);
  constexpr uint32_t fO = pack6(NONE, FA_S, FA_S, Q_PLUS, Q_QUAL, NONE);
  return c == E ? fE : c == G ? fG : c == A ? fA : fO;
}
G2S_FX_HD uint32_t apply(uint32_t f, uint32_t s) { return (f >> (3u * s)) & 7u; }
// first f, then g
G2S_FX_HD uint32_t compose(uint32_t f, uint32_t g) {
  uint32_t r = 0;
  for (uint32_t s = 0; s < kStates; s++) r |= apply(g, apply(f, s)) << (3u * s);
  return r;
}
// a line of class c read in state s opens a record (the record before it, if any, is complete)
G2S_FX_HD bool opens_record(uint32_t s, uint32_t c) { return (c == G && s <= FA_S) || (c == A && s == NONE); }
// the bytes of a line belong to the text when this is the state BEHIND the line
G2S_FX_HD bool is_sequence(uint32_t state_behind) { return state_behind == FA_S || state_behind == Q_PLUS; }

// The class of the line whose first byte is b0.  `b0_ends`: b0 is the line's '\n' (an empty line); b1_ends: the byte
// behind b0 is '\n' or the end of the file (so that a lone '\r' is the dropped one and the line is empty).
G2S_FX_HD uint32_t line_class(uint8_t b0, bool b1_ends) {
  if (b0 == '\n' || (b0 == '\r' && b1_ends)) return E;
  return b0 == '>' ? G : b0 == '@' ? A : O;
}
// the '\r' that parse_fastx drops: the last byte of its line
G2S_FX_HD bool dropped_cr(uint8_t b, bool next_ends) { return b == '\r' && next_ends; }

}  // namespace fastx
}  // namespace g2s
