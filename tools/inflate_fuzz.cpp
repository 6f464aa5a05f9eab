// tools/inflate_fuzz.cpp — gap2seq_amd/csrc/inflate_core.h compiled for the host under AddressSanitizer and
// UndefinedBehaviorSanitizer, against zlib: every member of the BGZF files named on the command line (the designed and
// corrupt members of tests/inflate_cases.py, exported by tools/inflate_fuzz.sh), then seeded random mutations of valid
// members.  For every input the two must agree on valid / not valid, and on every byte when valid.  Inputs and outputs
// live in heap blocks of exactly their size, so a read or write one byte out of bounds is reported.  CPU only.
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/inflate_fuzz.cpp -lz -o inflate_fuzz
//   ./inflate_fuzz [--mutations N] [--seed S] [file.bgzf ...]
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

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

int main(int argc, char** argv) {
  long mutations = 4000;
  uint64_t seed = 20240611;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--mutations") && i + 1 < argc) mutations = atol(argv[++i]);
    else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
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
  return 0;
}
