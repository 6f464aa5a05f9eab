// gap2seq_amd/csrc/fastx.hpp — FASTA/FASTQ text handling for the host side.
// Stands in for gatb BankFasta / BankAlbum as used at
// /root/reference/src/Gap2Seq.cpp:213 (reads), :224,:276-279,:426-431 (output),
// :287-289,:316-318 (scaffold iterator): multi-line records are joined, case is
// kept, the comment is the header line without '>', output is one line per
// sequence.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace g2s {

struct FastxRecord {
  std::string comment;
  std::string seq;
};

bool read_text_file(const std::string& path, std::string* out);
void parse_fastx(const std::string& text, std::vector<FastxRecord>* out);

// ---- gzip input (read files: GATB's bank reads .gz transparently).  Recognised by the magic bytes 1f 8b, never by name.
inline bool is_gzip(const uint8_t* p, size_t n) { return n >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
// A gzip stream of any number of members inflated by zlib, a buffer at a time.  The compressed bytes stay where they
// are (a mapped file, the caller's memory).  Strict: whatever follows a member must be another member, so trailing bytes
// that are none — the zero padding some tape and block writers leave, which gzip(1) ignores — are a corrupt stream.
class GzipReader {
 public:
  GzipReader(const uint8_t* bytes, size_t n);
  ~GzipReader();
  GzipReader(const GzipReader&) = delete;
  GzipReader& operator=(const GzipReader&) = delete;
  // up to cap inflated bytes into dst; fewer than cap only at the end of the stream.  false with *err set when the
  // stream is truncated or corrupt (a member's CRC and size are checked at its end).
  bool read(uint8_t* dst, size_t cap, size_t* got, std::string* err);
  bool at_end() const { return done_; }

 private:
  void* zs_ = nullptr;  // z_stream
  size_t left_ = 0;    // input bytes not yet handed to zlib
  bool done_ = false, in_member_ = false;
};
// A BAM file among the read files, told by its content alone: the bytes are gzip, their first member is a BGZF member (an
// extra subfield 'B','C'), and the inflated stream begins with "BAM\1".  Members are inflated until four bytes are known
// (n may be the head of a longer file: a member cut by n gives the bytes it has).  Any other gzip file is FASTA/FASTQ.
bool is_bam(const uint8_t* bytes, size_t n);
// a whole read file as text: its bytes, inflated when they are gzip.  *gz (may be null): whether they were.  false with
// *err naming the file when it cannot be read or its gzip stream is truncated or corrupt.
bool read_reads_file(const std::string& path, std::string* out, bool* gz, std::string* err);
bool reads_text_of_bytes(const uint8_t* bytes, size_t n, const std::string& name, std::string* out, bool* gz, std::string* err);
inline void append_fasta(std::string* out, const std::string& comment, const std::string& seq) {
  out->push_back('>');
  out->append(comment);
  out->push_back('\n');
  out->append(seq);
  out->push_back('\n');
}

// FASTA text whose records are ">comment\nSEQ\n" -> the same records with SEQ broken into lines of `width`
// characters (width <= 0: unchanged).  GATB's BankFasta, which the reference writes its output through
// (Gap2Seq.cpp:224,426-431), is recalled to break data lines at 70 columns unless told otherwise; that cannot
// be checked here (gatb-core is not part of the reference tree), so the command lines keep one line per
// record by default and offer -fasta-width 70.  Every FASTA reader of the pipeline accepts both.
inline std::string wrap_fasta(const char* text, size_t n, int width) {
  if (width <= 0) return std::string(text, n);
  std::string out;
  out.reserve(n + n / (size_t)width + 16);
  size_t i = 0;
  while (i < n) {
    size_t e = i;
    while (e < n && text[e] != '\n') e++;
    if (text[i] == '>') out.append(text + i, e - i);
    else {
      for (size_t p = i; p < e; p += (size_t)width) {
        if (p > i) out.push_back('\n');
        out.append(text + p, std::min<size_t>((size_t)width, e - p));
      }
    }
    out.push_back('\n');
    i = e + 1;
  }
  return out;
}

}  // namespace g2s
