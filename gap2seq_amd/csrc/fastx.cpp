// gap2seq_amd/csrc/fastx.cpp — see fastx.hpp.
#include "fastx.hpp"

#include <zlib.h>

#include <cstdio>
#include <cstring>

namespace g2s {

bool read_text_file(const std::string& path, std::string* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out->clear();
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, got);
  fclose(f);
  return true;
}

GzipReader::GzipReader(const uint8_t* bytes, size_t n) {
  z_stream* zs = new z_stream;
  memset(zs, 0, sizeof *zs);
  zs->next_in = const_cast<Bytef*>(bytes);
  zs->avail_in = 0;
  zs_ = zs;
  left_ = n;
  if (inflateInit2(zs, 16 + 15) != Z_OK) { delete zs; zs_ = nullptr; }
  done_ = n == 0;
}
GzipReader::~GzipReader() {
  if (zs_) { inflateEnd((z_stream*)zs_); delete (z_stream*)zs_; }
}
bool GzipReader::read(uint8_t* dst, size_t cap, size_t* got, std::string* err) {
  *got = 0;
  z_stream* zs = (z_stream*)zs_;
  if (!zs) { *err = "zlib could not be started"; return false; }
  while (*got < cap && !done_) {
    if (zs->avail_in == 0 && left_) {  // (avail_in is 32 bits wide: the input goes in by slices)
      const size_t step = std::min<size_t>(left_, (size_t)1 << 30);
      zs->avail_in = (uInt)step;
      left_ -= step;
    }
    if (!in_member_) {
      if (zs->avail_in == 0) { done_ = true; break; }
      if (inflateReset(zs) != Z_OK) { *err = "zlib could not be started"; return false; }
      in_member_ = true;
    }
    const size_t room = std::min<size_t>(cap - *got, (size_t)1 << 30);
    zs->next_out = dst + *got;
    zs->avail_out = (uInt)room;
    const int rc = ::inflate(zs, Z_NO_FLUSH);
    *got += room - zs->avail_out;
    if (rc == Z_STREAM_END) { in_member_ = false; continue; }
    if (rc == Z_BUF_ERROR && zs->avail_in == 0 && left_ == 0) { *err = "truncated gzip stream"; return false; }
    if (rc != Z_OK && rc != Z_BUF_ERROR) { *err = std::string("corrupt gzip stream (") + (zs->msg ? zs->msg : "zlib") + ")"; return false; }
    if (rc == Z_OK && zs->avail_in == 0 && left_ == 0 && zs->avail_out != 0) { *err = "truncated gzip stream"; return false; }
  }
  return true;
}

bool is_bam(const uint8_t* p, size_t n) {
  uint8_t head[4];
  size_t have = 0, o = 0;
  while (have < 4) {
    if (o + 18 > n || p[o] != 0x1f || p[o + 1] != 0x8b || p[o + 2] != 8 || !(p[o + 3] & 4)) return false;
    const size_t xlen = (size_t)p[o + 10] | (size_t)p[o + 11] << 8;
    if (o + 12 + xlen > n) return false;
    size_t bsize = 0;
    for (size_t x = o + 12; x + 4 <= o + 12 + xlen;) {
      const size_t slen = (size_t)p[x + 2] | (size_t)p[x + 3] << 8;
      if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) bsize = ((size_t)p[x + 4] | (size_t)p[x + 5] << 8) + 1;
      x += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || (p[o + 3] & ~4)) return false;
    const size_t data = o + 12 + xlen, data_end = std::min(o + bsize - 8, n);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef*>(p + data);
    zs.avail_in = (uInt)(data_end - data);
    zs.next_out = head + have;
    zs.avail_out = (uInt)(4 - have);
    const int rc = ::inflate(&zs, Z_SYNC_FLUSH);
    have = 4 - zs.avail_out;
    inflateEnd(&zs);
    if (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) return false;
    if (have < 4 && rc != Z_STREAM_END) return false;  // (a member that ends without its end: no BAM file)
    o += bsize;
  }
  return memcmp(head, "BAM\1", 4) == 0;
}

bool reads_text_of_bytes(const uint8_t* bytes, size_t n, const std::string& name, std::string* out, bool* gz, std::string* err) {
  if (gz) *gz = is_gzip(bytes, n);
  if (!is_gzip(bytes, n)) { out->assign((const char*)bytes, n); return true; }
  out->clear();
  GzipReader zr(bytes, n);
  std::vector<uint8_t> buf((size_t)1 << 20);
  while (!zr.at_end()) {
    size_t got = 0;
    std::string why;
    if (!zr.read(buf.data(), buf.size(), &got, &why)) { *err = name + ": " + why; return false; }
    out->append((const char*)buf.data(), got);
  }
  return true;
}
bool read_reads_file(const std::string& path, std::string* out, bool* gz, std::string* err) {
  std::string raw;
  if (!read_text_file(path, &raw)) { *err = "cannot read " + path; return false; }
  if (!is_gzip((const uint8_t*)raw.data(), raw.size())) { if (gz) *gz = false; out->swap(raw); return true; }
  return reads_text_of_bytes((const uint8_t*)raw.data(), raw.size(), path, out, gz, err);
}

namespace {
struct LineReader {
  const std::string& t;
  size_t pos = 0;
  explicit LineReader(const std::string& text) : t(text) {}
  bool next(const char** p, size_t* len) {
    if (pos >= t.size()) return false;
    size_t e = t.find('\n', pos);
    if (e == std::string::npos) e = t.size();
    *p = t.data() + pos;
    *len = e - pos;
    if (*len > 0 && (*p)[*len - 1] == '\r') (*len)--;
    pos = e + 1;
    return true;
  }
};
}  // namespace

void parse_fastx(const std::string& text, std::vector<FastxRecord>* out) {
  LineReader lr(text);
  const char* p;
  size_t len;
  FastxRecord* cur = nullptr;
  int fastq_line = -1;  // >=0 while inside a 4-line FASTQ record
  while (lr.next(&p, &len)) {
    if (fastq_line >= 0) {
      if (fastq_line == 0) cur->seq.assign(p, len);
      if (++fastq_line == 3) { fastq_line = -1; cur = nullptr; }
      continue;
    }
    if (len == 0) continue;
    if (p[0] == '>') {
      out->emplace_back();
      cur = &out->back();
      cur->comment.assign(p + 1, len - 1);
    } else if (p[0] == '@' && cur == nullptr) {
      out->emplace_back();
      cur = &out->back();
      cur->comment.assign(p + 1, len - 1);
      fastq_line = 0;
    } else if (cur) {
      cur->seq.append(p, len);
    }
  }
}

}  // namespace g2s
