// tools/inflate_fuzz.cpp — gap2seq_amd/csrc/inflate_core.h compiled for the host under AddressSanitizer and
// UndefinedBehaviorSanitizer, against zlib: every member of the BGZF files named on the command line (the designed and
// corrupt members of tests/inflate_cases.py, exported by tools/inflate_fuzz.sh), then seeded random mutations of valid
// members.  For every input the two must agree on valid / not valid, and on every byte when valid.  Inputs and outputs
// live in heap blocks of exactly their size, so a read or write one byte out of bounds is reported.  CPU only.
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/inflate_fuzz.cpp -lz -o inflate_fuzz
//   ./inflate_fuzz [--mutations N] [--seed S] [file.bgzf ...] [--deflate N stream.deflate ...]
// --deflate: the files behind it are raw deflate streams (the members of tests/gzip_cases.py's files) for
// gap2seq_amd/csrc/gzip_chunks.h: each goes through find / decode / chain / resolve at chunks of 1 and 4 KiB, every slot a
// heap block of exactly its capacity, then N seeded mutations of them do.  Every chunk must end in one of the five states;
// when every chunk ended ok up to a final block and no marker pointed in front of the stream, zlib must have read the same
// stream to the same bytes.  The 64-bit CRC shift is checked against the 32-bit one and against zlib's crc32_combine.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../gap2seq_amd/csrc/gzip_chunks.h"
#include "../gap2seq_amd/csrc/inflate_core.h"

namespace inf = g2s::inflate;

static bool by_zlib(const uint8_t* in, uint32_t n, uint32_t isize, uint32_t crc, std::vector<uint8_t>* out) {
  out->assign(isize, 0);
  if (isize == 0) return true;  // (as the reader: a member without bytes is not inflated)
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) abort();
  zs.next_in = const_cast<Bytef*>(in);
  zs.avail_in = n;
  zs.next_out = out->data();
  zs.avail_out = isize;
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
  inflateEnd(&zs);
  return ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), out->data(), isize) == crc;
}

static bool by_core(const uint8_t* in, uint32_t n, uint32_t isize, uint32_t crc, uint8_t** out) {
  *out = (uint8_t*)malloc(isize ? isize : 1);
  if (isize == 0) return true;
  uint8_t* src = (uint8_t*)malloc(n ? n : 1);  // (exactly n bytes: an over-read is out of bounds)
  if (n) memcpy(src, in, n);
  inf::Tables* T = new inf::Tables;
  inf::HostSink sink{*out};
  const uint32_t st = inf::inflate_member(src, n, isize, T, sink);
  delete T;
  free(src);
  return st == inf::kOk && inf::crc_by_slices(*out, isize) == crc;
}

static long g_valid = 0, g_invalid = 0;

static void check(const uint8_t* in, uint32_t n, uint32_t isize, uint32_t crc, const char* what) {
  if (isize > inf::kMaxMember) return;  // (the reader refuses such a file before anything is inflated)
  std::vector<uint8_t> a;
  uint8_t* b = nullptr;
  const bool za = by_zlib(in, n, isize, crc, &a), zb = by_core(in, n, isize, crc, &b);
  if (za != zb || (za && isize && memcmp(a.data(), b, isize) != 0)) {
    fprintf(stderr, "MISMATCH (%s): zlib %d, inflate_core %d, %u deflate bytes, isize %u\n", what, (int)za, (int)zb, n, isize);
    exit(1);
  }
  free(b);
  (za ? g_valid : g_invalid)++;
}

static void check_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + k);
  fclose(f);
  for (size_t o = 0; o + 26 <= d.size();) {
    const size_t xlen = d[o + 10] | d[o + 11] << 8, bsize = (size_t)(d[o + 16] | d[o + 17] << 8) + 1;
    if (o + bsize > d.size() || bsize < 12 + xlen + 8) { fprintf(stderr, "%s: not BGZF at %zu\n", path, o); exit(2); }
    uint32_t crc, isize;
    memcpy(&crc, &d[o + bsize - 8], 4);
    memcpy(&isize, &d[o + bsize - 4], 4);
    check(&d[o + 12 + xlen], (uint32_t)(bsize - 12 - xlen - 8), isize, crc, path);
    o += bsize;
  }
}

// ---- gzip_chunks.h
namespace gz = g2s::gzchunks;
static long g_chunk_runs = 0, g_chunk_done = 0, g_chunk_back = 0;

// zlib on a raw deflate stream: true with the bytes and the bytes of input consumed when it is one
static bool stream_by_zlib(const std::vector<uint8_t>& d, std::vector<uint8_t>* out, size_t* used) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) abort();
  zs.next_in = const_cast<Bytef*>(d.data());
  zs.avail_in = (uInt)d.size();
  out->clear();
  uint8_t buf[1 << 16];
  int rc = Z_OK;
  while (rc == Z_OK) {
    zs.next_out = buf;
    zs.avail_out = sizeof buf;
    rc = inflate(&zs, Z_NO_FLUSH);
    out->insert(out->end(), buf, buf + (sizeof buf - zs.avail_out));
    if (rc == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) break;  // (cut)
  }
  *used = zs.total_in;
  inflateEnd(&zs);
  return rc == Z_STREAM_END;
}

static void check_chunks(const std::vector<uint8_t>& d, uint32_t chunk, uint32_t ratio, const char* what) {
  if (d.empty()) return;
  const uint32_t n = (uint32_t)d.size();
  uint8_t* src = (uint8_t*)malloc(n);  // (exactly n bytes: an over-read is out of bounds)
  memcpy(src, d.data(), n);
  inf::Tables* T = new inf::Tables;
  const uint32_t nchunks = (n + chunk - 1) / chunk;
  std::vector<uint64_t> starts(nchunks, gz::kNoBit);
  starts[0] = 0;
  for (uint32_t c = 1; c < nchunks; c++)
    starts[c] = gz::find_start(src, n, (uint64_t)c * chunk * 8u, std::min<uint64_t>((uint64_t)(c + 1) * chunk, n) * 8u, T);
  std::vector<uint32_t> at;
  for (uint32_t c = 0; c < nchunks; c++)
    if (starts[c] != gz::kNoBit) at.push_back(c);
  std::vector<uint8_t> hist(gz::kWindow, 0), next(gz::kWindow), out;
  bool complete = false, bad = false;
  for (size_t i = 0; i < at.size(); i++) {
    const uint32_t behind = i + 1 < at.size() ? at[i + 1] : nchunks;
    const uint32_t cap = (behind - at[i]) * chunk * ratio;
    uint16_t* slot = (uint16_t*)malloc((size_t)cap * 2u);  // (exactly the capacity)
    gz::HostSymSink sink{slot};
    const gz::ChunkEnd e = gz::decode_chunk(src, n, starts[at[i]], i + 1 < at.size() ? starts[at[i + 1]] : gz::kNoBit, i == 0, cap, T, sink);
    if (e.status > gz::kEndCorrupt || e.out_n > cap) { fprintf(stderr, "NO STATUS (%s)\n", what); exit(1); }
    const bool go_on = e.status == gz::kEndOk || e.status == gz::kEndFinal;
    if (go_on) {
      const uint32_t valid = (uint32_t)std::min<size_t>(out.size(), gz::kWindow);
      for (uint32_t k = 0; k < e.out_n; k++) {
        bad = bad || !gz::sym_ok(slot[k], valid);
        out.push_back(gz::resolve_sym(slot[k], hist.data()));
      }
      for (uint32_t j = 0; j < gz::kWindow; j++) next[j] = gz::chain_byte(hist.data(), slot, e.out_n, j);
      hist.swap(next);
    }
    free(slot);
    if (!go_on) break;
    if (e.status == gz::kEndFinal) { complete = true; break; }
  }
  delete T;
  free(src);
  g_chunk_runs++;
  if (complete && !bad) {
    std::vector<uint8_t> z;
    size_t used = 0;
    if (!stream_by_zlib(d, &z, &used) || z != out) {
      fprintf(stderr, "MISMATCH (%s, chunks of %u): gzip_chunks.h completed %zu bytes, zlib did not read the same\n", what, chunk, out.size());
      exit(1);
    }
    const uint32_t head = (uint32_t)crc32(0L, out.data(), (uInt)std::min<size_t>(out.size(), 100));
    if (inf::crc_shift64(head, out.size()) != inf::crc_shift(head, (uint32_t)out.size())) {
      fprintf(stderr, "crc_shift64 is not crc_shift\n");
      exit(1);
    }
    g_chunk_done++;
  } else {
    g_chunk_back++;
  }
}

static std::vector<uint8_t> read_all(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + k);
  fclose(f);
  return d;
}

static void chunk_campaign(const std::vector<std::string>& paths, long mutations, uint64_t seed) {
  // the 64-bit shift beyond 4 GiB, against zlib's combination of a CRC with that of as many zero bytes ... which is what
  // a shift is when the piece behind has the CRC zlib gives zeros: CRC(A || Z) = shift(CRC(A), |Z|) ^ CRC(Z)
  for (uint64_t len : {(uint64_t)1, (uint64_t)4096, ((uint64_t)1 << 32) + 5u, ((uint64_t)3 << 33) + 12345u}) {
    const uint32_t a = 0xDEADBEEFu;
    const uint32_t want = (uint32_t)crc32_combine64(a, 0, (z_off64_t)len);  // (a piece behind with CRC 0: the pure shift)
    if (inf::crc_shift64(a, len) != want) { fprintf(stderr, "crc_shift64(%llu) is not zlib's\n", (unsigned long long)len); exit(1); }
  }
  std::vector<std::vector<uint8_t>> streams;
  for (const std::string& p : paths) streams.push_back(read_all(p.c_str()));
  for (size_t i = 0; i < streams.size(); i++)
    for (uint32_t chunk : {1024u, 4096u}) check_chunks(streams[i], chunk, 8, paths[i].c_str());
  std::mt19937_64 rng(seed);
  for (long it = 0; it < mutations && !streams.empty(); it++) {
    std::vector<uint8_t> d = streams[it % streams.size()];
    if (d.size() < 2) continue;
    switch (rng() % 6) {
      case 0: for (int k = 1 + (int)(rng() % 3); k; k--) d[rng() % d.size()] ^= (uint8_t)(1u << (rng() % 8)); break;
      case 1: d[rng() % d.size()] = (uint8_t)rng(); break;
      case 2: d.resize(1 + rng() % (d.size() - 1)); break;
      case 3: d.erase(d.begin(), d.begin() + (long)(rng() % (d.size() / 2)));  break;  // (a stream that begins anywhere)
      case 4: for (size_t k = rng() % d.size(), e = std::min(d.size(), k + 64); k < e; k++) d[k] = (uint8_t)rng(); break;
      default: for (size_t k = rng() % d.size(); k < d.size() && rng() % 4; k++) d[k] = (uint8_t)rng(); break;
    }
    check_chunks(d, rng() % 2 ? 1024u : 4096u, rng() % 4 ? 8u : 2u, "mutated");
  }
  printf("inflate_fuzz: gzip_chunks.h on %zu streams and %ld mutations: %ld runs, %ld completed as zlib reads them, %ld ended in a status\n",
         streams.size(), mutations, g_chunk_runs, g_chunk_done, g_chunk_back);
}

int main(int argc, char** argv) {
  long mutations = 4000;
  long chunk_mutations = -1;
  std::vector<std::string> deflate_paths;
  uint64_t seed = 20240611;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--mutations") && i + 1 < argc) mutations = atol(argv[++i]);
    else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--deflate") && i + 1 < argc) chunk_mutations = atol(argv[++i]);
    else if (chunk_mutations >= 0) deflate_paths.push_back(argv[i]);
    else check_file(argv[i]);
  }
  const long from_files = g_valid + g_invalid;
  std::mt19937_64 rng(seed);
  for (long it = 0; it < mutations; it++) {
    // a valid member: text, runs or noise, at some level and strategy
    const uint32_t size = (uint32_t)(rng() % (it % 50 == 0 ? 65537 : 3000));
    std::vector<uint8_t> p(size);
    const int kind = (int)(rng() % 3);
    for (uint32_t i = 0; i < size; i++)
      p[i] = kind == 0 ? (uint8_t)"ACGTN acgt\n"[rng() % 11] : kind == 1 ? (i && rng() % 40 ? p[i - 1] : (uint8_t)rng()) : (uint8_t)rng();
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    const int level = (int)(rng() % 10), strategy = rng() % 4 == 0 ? Z_FIXED : Z_DEFAULT_STRATEGY;
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 1 + (int)(rng() % 9), strategy) != Z_OK) abort();
    std::vector<uint8_t> d(deflateBound(&zs, size) + 16);
    zs.next_in = p.data();
    zs.avail_in = size;
    zs.next_out = d.data();
    zs.avail_out = (uInt)d.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
    d.resize(zs.total_out);
    deflateEnd(&zs);
    uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p.data(), size), isize = size;
    check(d.data(), (uint32_t)d.size(), isize, crc, "unchanged");
    // ... and a mutation of it
    switch (rng() % 6) {
      case 0: for (int k = 1 + (int)(rng() % 3); k; k--) d[rng() % d.size()] ^= (uint8_t)(1u << (rng() % 8)); break;
      case 1: d[rng() % d.size()] = (uint8_t)rng(); break;
      case 2: d.resize(rng() % d.size()); break;
      case 3: isize = (uint32_t)((int64_t)isize + (int64_t)(rng() % 5) - 2) & 0xFFFF; break;
      case 4: crc ^= 1u << (rng() % 32); break;
      default: for (size_t k = rng() % d.size(); k < d.size() && rng() % 4; k++) d[k] = (uint8_t)rng(); break;
    }
    check(d.data(), (uint32_t)d.size(), isize, crc, "mutated");
  }
  printf("inflate_fuzz: %ld members from files, %ld generated; %ld valid and %ld not valid, zlib and inflate_core.h agree on all\n",
         from_files, g_valid + g_invalid - from_files, g_valid, g_invalid);
  if (chunk_mutations >= 0) chunk_campaign(deflate_paths, chunk_mutations, seed);
  return 0;
}
