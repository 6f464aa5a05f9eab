// gap2seq_amd/csrc/reads_text.hip — see reads_text.h.  The build's text made on the device from the raw bytes of
// FASTA/FASTQ files: count / scan / write over the line state machine of fastx_machine.h, a piece of the file at a time.
//
// A piece is m bytes at a 16-byte boundary; unless it is the file's last, the byte behind it (raw[m], the halo) is
// there too — it is the first byte of the next piece, held back on the device so that a '\r' or a line head at a piece's
// end sees what follows it.  Per piece, on one stream, no kernel waits for another workgroup:
//   k_fastx_tile_fn     every 4 KiB tile's composed transition function
//   k_fastx_scan_fn     one workgroup: the state in front of every tile, from the carry's state
//   k_fastx_tile_count  every tile's text bytes and records, now that its state is known
//   k_fastx_scan_count  one workgroup: every tile's first output position inside the piece (32 bits)
//   k_fastx_write       the kept bytes and the separators to their 64-bit places in the text
//   k_fastx_carry       one thread: the carry for the next piece; at a file's end its last separator
// The carry (device memory, never read by the host between pieces) holds the machine's state, whether the next byte
// heads a line — a line may be longer than any number of pieces: bytes that head no line are the identity function, so
// the state behind the line's head simply flows through them — and where the file's text stands.
//
// A record's separator is written when the NEXT record's header is met; so that no position depends on "is this the
// file's first record" the kernels count the stream  N s0 N s1 ...  and write its byte j to text[base + j - 1]: byte 0
// falls away and the file's end writes the last N.
//
// A BAM file of the list (told by fastx.hpp: is_bam) takes no piece: Loader::run_bam_file has bam_reads.hip make its text
// behind what the list gave so far and moves the carry's text base past it — resident, or, for a file over the bound,
// streaming into a text sized from the file's inflated bytes.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bam_reads.h"
#include "bgzf_inflate.h"
#include "fastx.hpp"
#include "hip_host.h"
#include "inflate_core.h"
#include "reads_text.h"
#include "readfilter_gaps.hpp"

namespace {

namespace fx = g2s::fastx;

constexpr int FX_THREADS = 256;
constexpr int FX_RUN = 16;                       // bytes a lane
constexpr uint32_t FX_TILE = FX_THREADS * FX_RUN;  // bytes a workgroup
constexpr int FX_WAVES = FX_THREADS / 64;

struct FxCarry {
  uint64_t file_emit;  // bytes of this file's stream N s0 N s1 ... counted so far
  uint64_t base;       // where this file's text begins
  uint64_t records;    // all files
  uint32_t state, at_head;
  uint32_t overflow;   // a byte had no room in the text (the host's bound was wrong: never expected)
  uint32_t piece_state, piece_emit, piece_records;  // k_fastx_scan_fn / k_fastx_scan_count -> k_fastx_carry
};

// a lane's 16 bytes, the byte in front of them and the byte behind them
struct FxBytes {
  uint32_t w[4];
  uint32_t prev, next;
  __device__ __forceinline__ uint32_t at(int j) const { return j < FX_RUN ? (w[(j >> 2) & 3] >> (8 * (j & 3))) & 0xFFu : next; }
};

// `avail` bytes of raw are readable (m, and the halo unless the piece is its file's last); what lies behind them reads as
// '\n': the end of a file ends its last line.
__device__ __forceinline__ FxBytes fx_load(const uint8_t* __restrict__ raw, uint32_t g, uint32_t avail, uint32_t at_head) {
  FxBytes b;
  if (g + FX_RUN <= avail) {
    const uint4 v = *(const uint4*)(raw + g);
    b.w[0] = v.x; b.w[1] = v.y; b.w[2] = v.z; b.w[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t x = 0;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t i = g + 4 * q + r;
        x |= (uint32_t)(i < avail ? raw[i] : (uint8_t)'\n') << (8 * r);
      }
      b.w[q] = x;
    }
  }
  b.next = g + FX_RUN < avail ? raw[g + FX_RUN] : (uint32_t)'\n';
  b.prev = g == 0 ? (at_head ? (uint32_t)'\n' : 0u) : (g <= avail ? raw[g - 1] : 0u);
  return b;
}

// the composed transition function of the lane's bytes below m
__device__ __forceinline__ uint32_t fx_lane_fn(const FxBytes& b, uint32_t g, uint32_t m) {
  uint32_t f = fx::kIdentity, prev = b.prev;
#pragma unroll
  for (int j = 0; j < FX_RUN; j++) {
    const uint32_t c = b.at(j);
    if (g + j < m && prev == '\n') f = fx::compose(f, fx::line_fn(fx::line_class((uint8_t)c, b.at(j + 1) == '\n')));
    prev = c;
  }
  return f;
}

// the function of everything in the workgroup in front of this lane (*total: of the whole workgroup)
__device__ __forceinline__ uint32_t fx_block_exclusive_fn(uint32_t f, uint32_t* lds, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t x = f;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
    if (lane >= (uint32_t)d) x = fx::compose(y, x);
  }
  if (lane == 63) lds[wave] = x;
  uint32_t ex = (uint32_t)__shfl_up((int)x, 1, 64);
  if (lane == 0) ex = fx::kIdentity;
  __syncthreads();
  uint32_t pre = fx::kIdentity, all = fx::kIdentity;
#pragma unroll
  for (int wv = 0; wv < FX_WAVES; wv++) {
    if ((uint32_t)wv < wave) pre = fx::compose(pre, lds[wv]);
    all = fx::compose(all, lds[wv]);
  }
  __syncthreads();
  if (total) *total = all;
  return fx::compose(pre, ex);
}

// the sum of everything in the workgroup in front of this lane (*total: of the whole workgroup)
__device__ __forceinline__ uint32_t fx_block_exclusive_sum(uint32_t v, uint32_t* lds, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  uint32_t pre = 0, all = 0;
#pragma unroll
  for (int wv = 0; wv < FX_WAVES; wv++) {
    if ((uint32_t)wv < wave) pre += lds[wv];
    all += lds[wv];
  }
  __syncthreads();
  if (total) *total = all;
  return pre + x - v;
}

// The lane's bytes below m walked from state s.  Returns the text bytes they give (low 16 bits) and the records they open
// (high 16 bits).  WRITE: the bytes go to text[at + ...] (`at`: the stream position of the lane's first byte; stream
// byte 0 has no place), none at or beyond cap.
template <bool WRITE>
__device__ __forceinline__ uint32_t fx_walk(const FxBytes& b, uint32_t g, uint32_t m, uint32_t s, uint8_t* __restrict__ text,
                                            uint64_t origin, uint64_t at, uint64_t cap, uint32_t* overflow) {
  uint32_t emit = 0, rec = 0, prev = b.prev;
  auto put = [&](uint32_t c) {
    if constexpr (WRITE) {
      const uint64_t j = at + emit;
      if (j != 0) {
        const uint64_t to = origin + j - 1;
        if (to < cap) text[to] = (uint8_t)c;
        else *overflow = 1;
      }
    }
    emit++;
  };
#pragma unroll
  for (int j = 0; j < FX_RUN; j++) {
    const uint32_t c = b.at(j);
    const bool next_ends = b.at(j + 1) == '\n';
    if (g + j < m) {
      if (prev == '\n') {
        const uint32_t cls = fx::line_class((uint8_t)c, next_ends);
        if (fx::opens_record(s, cls)) { put('N'); rec++; }
        s = fx::apply(fx::line_fn(cls), s);
      }
      if (fx::is_sequence(s) && c != '\n' && !fx::dropped_cr((uint8_t)c, next_ends)) put(c);
    }
    prev = c;
  }
  return emit | rec << 16;
}

}  // namespace

__global__ __launch_bounds__(FX_THREADS) void k_fastx_tile_fn(const uint8_t* __restrict__ raw, uint32_t m, uint32_t avail,
                                                              const FxCarry* __restrict__ carry, uint32_t* __restrict__ tile_fn) {
  __shared__ uint32_t lds[FX_WAVES];
  const uint32_t g = blockIdx.x * FX_TILE + threadIdx.x * FX_RUN;
  const FxBytes b = fx_load(raw, g, avail, carry->at_head);
  uint32_t all;
  (void)fx_block_exclusive_fn(fx_lane_fn(b, g, m), lds, &all);
  if (threadIdx.x == 0) tile_fn[blockIdx.x] = all;
}

// one workgroup: tile_state[t] = the state in front of tile t
__global__ __launch_bounds__(FX_THREADS) void k_fastx_scan_fn(const uint32_t* __restrict__ tile_fn, uint32_t ntiles,
                                                              FxCarry* __restrict__ carry, uint32_t* __restrict__ tile_state) {
  __shared__ uint32_t lds[FX_WAVES];
  const uint32_t per = (ntiles + FX_THREADS - 1) / FX_THREADS;
  const uint32_t lo = min(threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
  uint32_t f = fx::kIdentity;
  for (uint32_t t = lo; t < hi; t++) f = fx::compose(f, tile_fn[t]);
  const uint32_t pre = fx_block_exclusive_fn(f, lds, nullptr);
  uint32_t s = fx::apply(pre, carry->state);
  for (uint32_t t = lo; t < hi; t++) {
    tile_state[t] = s;
    s = fx::apply(tile_fn[t], s);
  }
  if (threadIdx.x == FX_THREADS - 1) carry->piece_state = s;  // (its run is the last, or empty behind the last)
}

__global__ __launch_bounds__(FX_THREADS) void k_fastx_tile_count(const uint8_t* __restrict__ raw, uint32_t m, uint32_t avail,
                                                                 const FxCarry* __restrict__ carry,
                                                                 const uint32_t* __restrict__ tile_state,
                                                                 uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t lds[FX_WAVES];
  const uint32_t g = blockIdx.x * FX_TILE + threadIdx.x * FX_RUN;
  const FxBytes b = fx_load(raw, g, avail, carry->at_head);
  const uint32_t pre = fx_block_exclusive_fn(fx_lane_fn(b, g, m), lds, nullptr);
  const uint32_t s = fx::apply(pre, tile_state[blockIdx.x]);
  const uint32_t mine = fx_walk<false>(b, g, m, s, nullptr, 0, 0, 0, nullptr);
  uint32_t all;  // (a tile gives at most FX_TILE bytes and opens at most FX_TILE records: the halves do not meet)
  (void)fx_block_exclusive_sum(mine, lds, &all);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = all;
}

// one workgroup: tile_off[t] = the text bytes of the piece's tiles in front of t; the piece's totals
__global__ __launch_bounds__(FX_THREADS) void k_fastx_scan_count(const uint32_t* __restrict__ tile_count, uint32_t ntiles,
                                                                 FxCarry* __restrict__ carry, uint32_t* __restrict__ tile_off) {
  __shared__ uint32_t lds[FX_WAVES];
  const uint32_t per = (ntiles + FX_THREADS - 1) / FX_THREADS;
  const uint32_t lo = min(threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
  uint32_t emit = 0, rec = 0;
  for (uint32_t t = lo; t < hi; t++) { emit += tile_count[t] & 0xFFFFu; rec += tile_count[t] >> 16; }
  uint32_t all_emit, all_rec;
  uint32_t at = fx_block_exclusive_sum(emit, lds, &all_emit);
  (void)fx_block_exclusive_sum(rec, lds, &all_rec);
  for (uint32_t t = lo; t < hi; t++) {
    tile_off[t] = at;
    at += tile_count[t] & 0xFFFFu;
  }
  if (threadIdx.x == 0) { carry->piece_emit = all_emit; carry->piece_records = all_rec; }
}

__global__ __launch_bounds__(FX_THREADS) void k_fastx_write(const uint8_t* __restrict__ raw, uint32_t m, uint32_t avail,
                                                            FxCarry* __restrict__ carry, const uint32_t* __restrict__ tile_state,
                                                            const uint32_t* __restrict__ tile_off, uint8_t* __restrict__ text,
                                                            uint64_t cap) {
  __shared__ uint32_t lds[FX_WAVES];
  const uint32_t g = blockIdx.x * FX_TILE + threadIdx.x * FX_RUN;
  const FxBytes b = fx_load(raw, g, avail, carry->at_head);
  const uint32_t pre = fx_block_exclusive_fn(fx_lane_fn(b, g, m), lds, nullptr);
  const uint32_t s = fx::apply(pre, tile_state[blockIdx.x]);
  const uint32_t mine = fx_walk<false>(b, g, m, s, nullptr, 0, 0, 0, nullptr) & 0xFFFFu;
  const uint32_t in_tile = fx_block_exclusive_sum(mine, lds, nullptr);
  if (mine == 0) return;
  uint32_t over = 0;
  (void)fx_walk<true>(b, g, m, s, text, carry->base, carry->file_emit + tile_off[blockIdx.x] + in_tile, cap, &over);
  if (over) carry->overflow = 1;
}

// one thread, behind k_fastx_write.  ran: the piece had bytes (the kernels above ran); last: it ends its file
__global__ void k_fastx_carry(const uint8_t* __restrict__ raw, uint32_t m, int ran, int last, FxCarry* __restrict__ carry,
                              uint8_t* __restrict__ text, uint64_t cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  FxCarry c = *carry;
  if (ran) {
    c.state = c.piece_state;
    c.at_head = raw[m - 1] == '\n';
    c.file_emit += c.piece_emit;
    c.records += c.piece_records;
  }
  if (last) {
    if (c.file_emit) {
      const uint64_t to = c.base + c.file_emit - 1;
      if (to < cap) text[to] = 'N';
      else c.overflow = 1;
    }
    c.base += c.file_emit;
    c.file_emit = 0;
    c.state = fx::NONE;
    c.at_head = 1;
  }
  c.piece_state = c.piece_emit = c.piece_records = 0;
  *carry = c;
}

__global__ void k_fastx_fill(uint8_t* __restrict__ p, uint64_t n, uint8_t v) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = v;
}

namespace g2s {

uint64_t device_text_bytes(uint64_t T) {
  // (solid_passes.h: PB_TILE = 256 * 64 start positions a tile, PB_HALO = 128; restated in dbg_gpu.hip's static_assert)
  constexpr uint64_t tile = 256 * 64, halo = 128;
  return (T + tile - 1) / tile * tile + halo;
}

void free_device_text(DeviceText* t) {
  if (t->d_text && hipSetDevice(t->device) == hipSuccess) (void)hipFree(t->d_text);
  *t = DeviceText();
}

void machine_text_host(const uint8_t* bytes, size_t n, std::string* out, uint64_t* records) {
  uint32_t s = fx::NONE;
  bool any = false;
  size_t i = 0;
  while (i < n) {
    size_t e = i;
    while (e < n && bytes[e] != '\n') e++;
    const bool b1_ends = i + 1 >= n || bytes[i + 1] == '\n';
    const uint32_t cls = fx::line_class(i < e ? bytes[i] : (uint8_t)'\n', b1_ends);
    if (fx::opens_record(s, cls)) {
      if (any) out->push_back('N');
      any = true;
      if (records) ++*records;
    }
    s = fx::apply(fx::line_fn(cls), s);
    if (fx::is_sequence(s))
      for (size_t j = i; j < e; j++)
        if (!fx::dropped_cr(bytes[j], j + 1 == e)) out->push_back((char)bytes[j]);
    i = e + 1;
  }
  if (any) out->push_back('N');
}

namespace {

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// one input opened: a plain file is read piece by piece; a gzip file is mapped (its compressed bytes are read in place)
struct OpenInput {
  std::string name;
  const uint8_t* mem = nullptr;
  size_t n = 0, at = 0;
  int fd = -1;
  void* map = nullptr;
  size_t map_len = 0;
  bool gz = false;
  ~OpenInput() {
    if (map) munmap(map, map_len);
    if (fd >= 0) ::close(fd);
  }
  bool open(const ReadsInput& in, std::string* err) {
    if (in.mem || in.path.empty()) {
      name = in.path.empty() ? "(memory)" : in.path;
      mem = in.mem;
      n = in.mem_n;
      gz = is_gzip(mem, n);
      return true;
    }
    name = in.path;
    fd = ::open(in.path.c_str(), O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { *err = "cannot read " + in.path; return false; }
    n = (size_t)st.st_size;
    uint8_t magic[2] = {0, 0};
    if (n >= 2 && pread(fd, magic, 2, 0) != 2) { *err = "cannot read " + in.path; return false; }
    gz = is_gzip(magic, n);
    if (gz) {
      void* p = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
      if (p == MAP_FAILED) { *err = "cannot map " + in.path; return false; }
      map = p;
      map_len = n;
      madvise(p, n, MADV_SEQUENTIAL);
      mem = (const uint8_t*)p;
    }
    return true;
  }
  // plain input: up to cap bytes; fewer than cap only at the end
  bool read_plain(uint8_t* dst, size_t cap, size_t* got, std::string* err) {
    *got = 0;
    if (mem) {
      *got = std::min(cap, n - at);
      memcpy(dst, mem + at, *got);
      at += *got;
      return true;
    }
    while (*got < cap) {
      const ssize_t r = ::read(fd, dst + *got, cap - *got);
      if (r < 0) { *err = "cannot read " + name; return false; }
      if (r == 0) break;
      *got += (size_t)r;
    }
    return true;
  }
};

// a BGZF member at p[0 .. left): its size, where its deflate bytes begin; false when it is none (no BC subfield, or cut)
bool bgzf_member(const uint8_t* p, size_t left, size_t* bsize, size_t* data_off) {
  if (left < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
  const size_t xlen = rd16(p + 10);
  if (12 + xlen > left) return false;
  size_t bs = 0;
  for (size_t x = 12; x + 4 <= 12 + xlen;) {
    const size_t slen = rd16(p + x + 2);
    if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bs = (size_t)rd16(p + x + 4) + 1;
    x += 4 + slen;
  }
  if (bs < 12 + xlen + 8 || bs > left) return false;
  if (p[3] & ~4) return false;  // (a name, a comment or a header CRC in front of the deflate bytes: zlib reads those)
  if (rd32(p + bs - 4) > inflate::kMaxMember) return false;
  *bsize = bs;
  *data_off = 12 + xlen;
  return true;
}

struct Loader {
  int device = 0;
  size_t piece = 0, raw_cap = 0;
  uint64_t first_cap = 0;
  bool host_inflate = false;
  size_t bam_window = 0;       // a BAM file's window: the piece as asked for (0: the reader's own)
  uint64_t resident_cap = 0;   // G2S_BUILD_RESIDENT_CAP
  uint64_t mem_limit = 0;      // half the free device memory when the loader began, and the cap
  int bam_stream = -1;         // G2S_BUILD_BAM_STREAM: 1 the streaming form always, 0 never, -1 when resident does not fit
  uint64_t bam_by_host = 0;    // BAM files whose text the host walk made (host_inflate)
  ReadsLoadInfo* info = nullptr;
  std::string* why = nullptr;  // (G2S_HIP_TRY)
  std::string io_error;

  hipStream_t own = nullptr, cur = nullptr;
  // (one allocation each for the two raw buffers, for the carry and the tile arrays, and for the two staging buffers:
  // on a small file the calls that make and free them are what the loader costs)
  DevMem d_raw_both, d_work, d_text, d_held;
  bool device_gzip = false;    // gzip files that are no BGZF files take the chunked device inflate (gzip_inflate.h)
  PinMem h_both;
  struct Part {
    void* p = nullptr;
    template <class T> T* as() const { return (T*)p; }
  } d_raw[2], d_carry, d_tile_fn, d_tile_state, d_tile_count, d_tile_off, h_raw[2];
  DevEvent done[2];
  bool used[2] = {false, false};
  std::unique_ptr<BgzfDevice> bg;
  size_t bg_members[2] = {0, 0};  // members of the window in flight in each of bg's slots
  size_t bg_max_out = 0, bg_max_in = 0, bg_max_members = 0;
  uint64_t cap = 0, bound = 0;
  int slot = 0;
  bool have_front = false;
  size_t halo_at = 0;  // index of the held-back byte in the other slot's raw buffer

  // (own is the null stream, as for the rest of the build: making and destroying a stream costs more than a small
  // file's whole load; a BGZF file's pieces run on the device inflate's stream)
  ~Loader() {
    (void)hipStreamSynchronize(cur);
    bg.reset();
  }

  bool init(uint64_t cap0) {
    G2S_HIP_TRY(hipSetDevice(device));
    bg_max_out = std::max<size_t>(piece, inflate::kMaxMember);
    raw_cap = bg_max_out + 1 + 16;
    const size_t max_tiles = raw_cap / FX_TILE + 2;
    const size_t raw_stride = (raw_cap + 255) & ~(size_t)255, tiles_stride = (max_tiles * 4 + 255) & ~(size_t)255;
    G2S_HIP_TRY(d_raw_both.alloc(2 * raw_stride));
    G2S_HIP_TRY(d_work.alloc(256 + 4 * tiles_stride));
    for (int b = 0; b < 2; b++) {
      d_raw[b].p = d_raw_both.as<uint8_t>() + (size_t)b * raw_stride;
      G2S_HIP_TRY(done[b].create());
    }
    static_assert(sizeof(FxCarry) <= 256, "the carry's place in d_work");
    d_carry.p = d_work.p;
    d_tile_fn.p = d_work.as<uint8_t>() + 256;
    d_tile_state.p = d_work.as<uint8_t>() + 256 + tiles_stride;
    d_tile_count.p = d_work.as<uint8_t>() + 256 + 2 * tiles_stride;
    d_tile_off.p = d_work.as<uint8_t>() + 256 + 3 * tiles_stride;
    FxCarry c;
    memset(&c, 0, sizeof c);
    c.at_head = 1;
    G2S_HIP_TRY(hipMemcpy(d_carry.p, &c, sizeof c, hipMemcpyHostToDevice));
    cap = std::max<uint64_t>(cap0, 16);
    G2S_HIP_TRY(d_text.alloc((size_t)cap));
    return true;
  }

  bool use_stream(hipStream_t s) {
    if (s != cur) {
      G2S_HIP_TRY(hipStreamSynchronize(cur));
      cur = s;
    }
    return true;
  }

  bool read_carry(FxCarry* c) {
    G2S_HIP_TRY(hipStreamSynchronize(cur));
    G2S_HIP_TRY(hipMemcpy(c, d_carry.p, sizeof *c, hipMemcpyDeviceToHost));
    return true;
  }

  // room for `more` further text bytes (an upper bound of what the next piece gives)
  bool reserve(uint64_t more) {
    if (bound + more + 1 <= cap) { bound += more; return true; }
    FxCarry c;
    if (!read_carry(&c)) return false;
    const uint64_t have = c.base + c.file_emit;  // (the true position: the bound counts every raw byte)
    bound = have;
    if (have + more + 1 > cap && !grow(std::max<uint64_t>(2 * cap, have + more + 1), have)) return false;
    bound += more;
    return true;
  }
  bool grow(uint64_t new_cap, uint64_t have) {
    DevMem bigger;
    G2S_HIP_TRY(bigger.alloc((size_t)new_cap));
    if (have) G2S_HIP_TRY(hipMemcpy(bigger.p, d_text.p, (size_t)std::min(have, cap), hipMemcpyDeviceToDevice));
    d_text = std::move(bigger);
    cap = new_cap;
    info->grows++;
    return true;
  }

  // room for a BAM file's `more` text bytes behind the `have` there are: sized from the count, once, padding included
  bool room(uint64_t have, uint64_t more) {
    const uint64_t need = device_text_bytes(have + more);
    if (need <= cap) return true;
    DevMem bigger;
    G2S_HIP_TRY(bigger.alloc((size_t)need));
    if (have) G2S_HIP_TRY(hipMemcpy(bigger.p, d_text.p, (size_t)std::min(have, cap), hipMemcpyDeviceToDevice));
    d_text = std::move(bigger);
    cap = need;
    return true;
  }

  // One BAM file (bam_reads.h): its text behind what the list has given so far, and the carry's text base moved past
  // it, so that a FASTA/FASTQ file behind it lands in the right place.  The resident stream and the rows are gone when
  // this returns.  kReadsOk, kReadsGaveUp (*why, info->bam_reason) or kReadsIoError (io_error).
  ReadsLoadResult run_bam_file(const ReadsInput& in, int* how) {
    FxCarry c;
    if (!read_carry(&c)) return kReadsGaveUp;  // (waits for the files in front; between files file_emit is 0)
    const uint64_t have = c.base;
    uint64_t kept = 0, skipped = 0, bytes = 0;
    info->bam_files++;
    auto gave_up = [&](int reason, int anomaly, const std::string& w) {
      info->bam_reason = reason;
      info->bam_anomaly = anomaly;
      if (why) *why = w;
      return kReadsGaveUp;
    };
    if (host_inflate) {  // (zlib and the host walk; the text is copied up and the list goes on)
      std::vector<std::string> seqs;
      uint64_t raw = 0;
      if (!bam_reads_host(in, &seqs, &skipped, &raw, &io_error)) return kReadsIoError;
      std::string text;
      for (const std::string& q : seqs) { text += q; text.push_back('N'); }
      bytes = text.size();
      kept = seqs.size();
      if (!room(have, bytes)) return gave_up(kBamReadsHip, 0, why ? *why : std::string());
      if (bytes) G2S_HIP_TRY_AS(hipMemcpy(d_text.as<uint8_t>() + have, text.data(), text.size(), hipMemcpyHostToDevice),
                                (hip_fail(why, what_, e_), info->bam_reason = kBamReadsHip, kReadsGaveUp));
      info->raw_bytes += raw;
      bam_by_host++;
      *how = kInflateZlib;
    } else {
      BamReadsDevice B;
      int reason = kBamReadsHip, anomaly = 0;
      std::string w;
      bool stream = bam_stream == 1;
      if (!stream) {
        const BamReadsDevice::Result r = B.prepare(in, device, bam_window, resident_cap, &reason, &anomaly, &w);
        if (r == BamReadsDevice::kIoError) { io_error = w; return kReadsIoError; }
        if (r == BamReadsDevice::kOk) {
          bytes = B.text_bytes();
          if (B.resident_bytes() + device_text_bytes(have + bytes) > mem_limit) {
            if (bam_stream == 0) return gave_up(kBamReadsOverCap, 0, "a BAM file's stream, rows and text are over the cap");
            stream = true;
          }
        } else if (bam_stream != 0 && B.resident_did_not_fit()) {
          stream = true;
        } else {
          return gave_up(reason, anomaly, w);
        }
      }
      if (stream) {
        // everything the streaming form holds counts against the limit: the fixed part and the text, whose capacity
        // comes from the bound of two thirds of the stream behind the header, or from what the limit leaves
        const BamReadsDevice::Result o = B.stream_open(in, device, bam_window, &w);
        if (o == BamReadsDevice::kIoError) { io_error = w; return kReadsIoError; }
        if (o != BamReadsDevice::kOk) return gave_up(kBamReadsHip, 0, w);
        const uint64_t fixed = B.stream_fixed_bytes(), pad = device_text_bytes(0), tile = device_text_bytes(1) - pad;
        const uint64_t left = mem_limit > fixed + pad ? (mem_limit - fixed - pad) / tile * tile : 0;  // text positions
        if (left <= have) return gave_up(kBamReadsOverCap, 0, "a BAM file's windows and text are over the cap");
        const uint64_t most = std::min<uint64_t>(2 * B.stream_payload() / 3, left - have);
        if (!room(have, most)) return gave_up(kBamReadsHip, 0, why ? *why : std::string());
        // (the bound is the text's, not the buffer's: its padding stays free, so the text's end needs no larger one)
        const BamReadsDevice::Result r = B.stream_run(d_text.as<uint8_t>(), have, have + most, bam_window, &reason, &anomaly, &w);
        if (r != BamReadsDevice::kOk) return gave_up(reason, anomaly, w);
        bytes = B.text_bytes();
        info->bam_streamed++;
        info->bam_stream_windows += B.windows();
        info->bam_stream_peak = std::max<uint64_t>(info->bam_stream_peak, fixed + cap);
      } else {
        if (!room(have, bytes)) return gave_up(kBamReadsHip, 0, why ? *why : std::string());
        if (!B.write(d_text.as<uint8_t>(), have, cap, &w)) return gave_up(kBamReadsHip, 0, w);
      }
      kept = B.kept();
      skipped = B.skipped();
      info->pieces += B.windows();
      info->raw_bytes += B.stream_bytes();
      *how = kInflateDevice;
    }
    c.base = have + bytes;
    c.records += kept;
    G2S_HIP_TRY_AS(hipMemcpy(d_carry.p, &c, sizeof c, hipMemcpyHostToDevice), (hip_fail(why, what_, e_), info->bam_reason = kBamReadsHip, kReadsGaveUp));
    bound = c.base;
    info->bam_kept += kept;
    info->bam_skipped += skipped;
    return kReadsOk;
  }

  // the kernels of one piece: m bytes at raw (a 16-byte boundary), the halo behind them unless `last`
  bool run_piece(const uint8_t* raw, uint32_t m, bool last) {
    FxCarry* carry = d_carry.as<FxCarry>();
    if (m) {
      const uint32_t avail = last ? m : m + 1, ntiles = (m + FX_TILE - 1) / FX_TILE;
      hipLaunchKernelGGL(k_fastx_tile_fn, dim3(ntiles), dim3(FX_THREADS), 0, cur, raw, m, avail, (const FxCarry*)carry,
                         d_tile_fn.as<uint32_t>());
      hipLaunchKernelGGL(k_fastx_scan_fn, dim3(1), dim3(FX_THREADS), 0, cur, (const uint32_t*)d_tile_fn.p, ntiles, carry,
                         d_tile_state.as<uint32_t>());
      hipLaunchKernelGGL(k_fastx_tile_count, dim3(ntiles), dim3(FX_THREADS), 0, cur, raw, m, avail, (const FxCarry*)carry,
                         (const uint32_t*)d_tile_state.p, d_tile_count.as<uint32_t>());
      hipLaunchKernelGGL(k_fastx_scan_count, dim3(1), dim3(FX_THREADS), 0, cur, (const uint32_t*)d_tile_count.p, ntiles, carry,
                         d_tile_off.as<uint32_t>());
      hipLaunchKernelGGL(k_fastx_write, dim3(ntiles), dim3(FX_THREADS), 0, cur, raw, m, avail, carry,
                         (const uint32_t*)d_tile_state.p, (const uint32_t*)d_tile_off.p, d_text.as<uint8_t>(), cap);
    }
    if (m || last)
      hipLaunchKernelGGL(k_fastx_carry, dim3(1), dim3(64), 0, cur, raw, m, m ? 1 : 0, last ? 1 : 0, carry, d_text.as<uint8_t>(), cap);
    G2S_HIP_TRY(hipGetLastError());
    info->pieces++;
    return true;
  }

  // the window that went through bg's slot b has been inflated: its members' status words
  enum Check { kGood, kCorrupt, kRefused };
  Check check_window(int b) {
    if (!bg || !bg_members[b]) return kGood;
    const size_t nm = bg_members[b];
    bg_members[b] = 0;
    if (!bg->wait(b, why)) return kRefused;
    for (size_t i = 0; i < nm; i++)
      if (bg->status(b)[i] != inflate::kOk) return kCorrupt;
    return kGood;
  }

  bool make_bgzf() {
    if (bg) return true;
    bg_max_members = bg_max_out / 1024 + 64;
    bg_max_in = bg_max_out + bg_max_members * 16 + inflate::kMaxMember;
    std::string w;
    bg.reset(BgzfDevice::create(device, bg_max_in, bg_max_out, bg_max_members, 0, &w, false));
    if (!bg && why) *why = "BGZF inflate: " + w;
    return bg != nullptr;
  }

  // A gzip file that is no BGZF file, inflated chunk by chunk on the device (gzip_inflate.h): every window's resolved
  // bytes go through run_piece where they lie, in pieces of at most `piece` bytes, the byte a window holds back for the
  // next one kept in d_held.  *done: the route completed the file.  Else the text position, the carry and the counts
  // are back where the file began, and zlib reads it.  False only when the loader itself cannot go on (*why).
  bool run_gzip_device(const OpenInput& f, bool* done) {
    *done = false;
    FxCarry c0;
    if (!use_stream(own) || !read_carry(&c0)) return false;
    const uint64_t bound0 = bound, pieces0 = info->pieces, raw0 = info->raw_bytes;
    GzipParams P = gzip_params_from_env();
    P.quarter_rule = true;
    // the window's buffers count against the loader's bound beside the text; W from what it leaves
    P.window_chunks = (uint32_t)std::min<uint64_t>(P.window_chunks, std::max<uint64_t>((f.n + P.chunk - 1) / P.chunk, 2));
    const uint64_t room = mem_limit > cap ? mem_limit - cap : 0;
    while (P.window_chunks > 2 && gzip_device_bytes(P) > room) P.window_chunks = std::max<uint32_t>(P.window_chunks / 2, 2);
    info->gzip.files++;
    auto give_back = [&](int outcome) {
      info->gzip.outcome = outcome;
      if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s]   %s: the device gzip route gave the file back (outcome %d)\n", f.name.c_str(), outcome);
      // (what the route wrote behind the file's first text position is overwritten by what zlib gives)
      G2S_HIP_TRY(hipStreamSynchronize(cur));
      G2S_HIP_TRY(hipMemcpy(d_carry.p, &c0, sizeof c0, hipMemcpyHostToDevice));
      bound = bound0;
      info->pieces = pieces0;
      info->raw_bytes = raw0;
      have_front = false;
      return true;
    };
    if (gzip_device_bytes(P) > room) return give_back(kGzMemory);
    std::string w;
    std::unique_ptr<GzipBackend> B = make_gzip_device_backend(device, cur, P, &w);
    if (!B) return give_back(kGzHip);
    info->gzip.peak_device_bytes = std::max<uint64_t>(info->gzip.peak_device_bytes, B->device_bytes());
    if (!d_held.p) G2S_HIP_TRY(d_held.alloc(16));
    const size_t step = std::max<size_t>(piece & ~(size_t)15, 16);
    bool failed = false;
    GzipStats st;
    const int outcome = gzip_route(
        f.mem, f.n, P, *B, &st, [&]() -> uint32_t { return have_front ? 1u : 0u; },
        [&](const uint8_t* bytes, uint64_t n_new, bool last) -> bool {
          const uint32_t front = have_front ? 1u : 0u;
          uint8_t* raw = const_cast<uint8_t*>(bytes) - front;
          const uint64_t total = front + n_new;
          if (total == 0 && !last) return true;
          if (front) G2S_HIP_TRY_AS(hipMemcpyAsync(raw, d_held.p, 1, hipMemcpyDeviceToDevice, cur), (hip_fail(why, what_, e_), failed = true, false));
          const uint64_t M = last ? total : total - 1;  // (the last byte is held back: it is the next window's halo)
          for (uint64_t o = 0; o < M || (last && o == 0); o += step) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(step, M - o);
            if (!reserve(m) || !run_piece(raw + o, m, last && o + m == M)) { failed = true; return false; }
            if (M == 0) break;
          }
          if (!last) G2S_HIP_TRY_AS(hipMemcpyAsync(d_held.p, raw + M, 1, hipMemcpyDeviceToDevice, cur), (hip_fail(why, what_, e_), failed = true, false));
          info->raw_bytes += n_new;
          have_front = !last;
          return true;
        });
    info->gzip.windows += st.windows;
    info->gzip.chunks += st.chunks;
    info->gzip.starts_found += st.starts_found;
    info->gzip.absorbed += st.absorbed;
    if (failed) return false;  // (a HIP call of the loader's own failed: the host loader takes over)
    if (outcome != kGzDone) {
      if (outcome == kGzHip && why) *why = B->why;
      return give_back(outcome);
    }
    info->gzip.members += st.members;
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s]   %s: inflated on the device, %llu members in %llu windows, %llu chunks with %llu starts found\n", f.name.c_str(),
              (unsigned long long)st.members, (unsigned long long)st.windows, (unsigned long long)st.chunks, (unsigned long long)st.starts_found);
    G2S_HIP_TRY(hipStreamSynchronize(cur));  // (the pieces read the backend's buffer, which goes with B)
    have_front = false;
    *done = true;
    return true;
  }

  // One file.  kReadsOk, kReadsGaveUp (*why) or kReadsIoError (io_error).
  ReadsLoadResult run_file(const ReadsInput& in, int* how) {
    OpenInput f;
    if (!f.open(in, &io_error)) return kReadsIoError;
    if (f.gz && is_bam(f.mem, f.n)) {  // (read where it is mapped, under the file's name)
      ReadsInput mapped;
      mapped.path = f.name;
      mapped.mem = f.mem;
      mapped.mem_n = f.n;
      return run_bam_file(mapped, how);
    }
    enum { PLAIN, ZLIB, BGZF, DEVGZ } mode = !f.gz ? PLAIN : ZLIB;
    size_t bsize = 0, doff = 0;
    if (f.gz && !host_inflate && bgzf_member(f.mem, f.n, &bsize, &doff)) mode = BGZF;
    else if (f.gz && !host_inflate && device_gzip) mode = DEVGZ;
    if (mode == DEVGZ) {
      bool done = false;
      if (!run_gzip_device(f, &done)) return kReadsGaveUp;
      if (done) { *how = kInflateDeviceGzip; return kReadsOk; }
      mode = ZLIB;  // (given back: zlib reads the file from its first byte, and says what is wrong with it if anything is)
    }
    std::unique_ptr<GzipReader> zr;
    if (mode == ZLIB) zr.reset(new GzipReader(f.mem, f.n));
    bool used_zlib = false, used_dev = false;
    auto corrupt = [&](const std::string& what) { io_error = f.name + ": " + what; return kReadsIoError; };
    for (;;) {
      const int b = slot;
      if (used[b]) G2S_HIP_TRY_AS(hipEventSynchronize(done[b].e), (hip_fail(why, what_, e_), kReadsGaveUp));
      switch (check_window(b)) {
        case kCorrupt: return corrupt("corrupt BGZF member");
        case kRefused: return kReadsGaveUp;
        default: break;
      }
      const size_t front = have_front ? 1 : 0;
      size_t n_new = 0, n_members = 0, in_bytes = 0;
      bool last = false;
      if (mode == BGZF) {
        if (f.at < f.n && !bgzf_member(f.mem + f.at, f.n - f.at, &bsize, &doff)) {
          if (!is_gzip(f.mem + f.at, f.n - f.at) || f.n - f.at < 18) return corrupt("truncated or corrupt gzip stream");
          mode = ZLIB;  // (no BGZF member from here on: zlib says what it is)
          zr.reset(new GzipReader(f.mem + f.at, f.n - f.at));
        } else {
          if (!make_bgzf()) return kReadsGaveUp;
          BgzfMember* M = bg->members(b);
          uint8_t* hin = bg->in(b);
          // (a window: whole members up to a piece of inflated bytes, one member at the least)
          while (f.at < f.n && bgzf_member(f.mem + f.at, f.n - f.at, &bsize, &doff)) {
            const uint8_t* blk = f.mem + f.at;
            const uint32_t dl = (uint32_t)(bsize - doff - 8), isize = rd32(blk + bsize - 4);
            const size_t padded = ((size_t)dl + 15) & ~(size_t)15;
            if (n_members && (n_new + isize > piece || n_members == bg_max_members || in_bytes + padded > bg_max_in)) break;
            M[n_members++] = BgzfMember{in_bytes, n_new, dl, isize, rd32(blk + bsize - 8), 0};
            if (isize) {
              memcpy(hin + in_bytes, blk + doff, dl);
              in_bytes += padded;
            }
            n_new += isize;
            f.at += bsize;
          }
          last = f.at >= f.n;
          used_dev = true;
        }
      }
      if (mode != BGZF) {
        std::string w;
        // (page-locked staging is made when the first piece needs it: a BGZF file's bytes are staged by bgzf_inflate.h)
        if (!h_both.p) {
          G2S_HIP_TRY_AS(h_both.alloc(2 * piece), (hip_fail(why, what_, e_), kReadsGaveUp));
          h_raw[0].p = h_both.p;
          h_raw[1].p = (uint8_t*)h_both.p + piece;
        }
        if (mode == ZLIB) {
          if (!zr->read((uint8_t*)h_raw[b].p, piece, &n_new, &w)) return corrupt(w);
          last = zr->at_end();
          used_zlib = true;
        } else {
          if (!f.read_plain((uint8_t*)h_raw[b].p, piece, &n_new, &io_error)) return kReadsIoError;
          last = n_new < piece;
        }
      }
      if (!last && n_new == 0) continue;  // (members without bytes)
      if (front + n_new > raw_cap - 16 || front + n_new >= (1ull << 31)) { if (why) *why = "a piece larger than its buffer"; return kReadsGaveUp; }
      uint8_t* raw = d_raw[b].as<uint8_t>();
      if (mode == BGZF) {
        if (!use_stream((hipStream_t)bg->stream())) return kReadsGaveUp;
      } else if (!use_stream(own)) {
        return kReadsGaveUp;
      }
      if (front) G2S_HIP_TRY_AS(hipMemcpyAsync(raw, d_raw[b ^ 1].as<uint8_t>() + halo_at, 1, hipMemcpyDeviceToDevice, cur), (hip_fail(why, what_, e_), kReadsGaveUp));
      if (mode == BGZF) {
        if (n_members) {
          if (!bg->launch(b, n_members, in_bytes, n_new, why, false, raw + front)) return kReadsGaveUp;
          bg_members[b] = n_members;
        }
      } else if (n_new) {
        G2S_HIP_TRY_AS(hipMemcpyAsync(raw + front, h_raw[b].p, n_new, hipMemcpyHostToDevice, cur), (hip_fail(why, what_, e_), kReadsGaveUp));
      }
      const size_t availb = front + n_new;
      const uint32_t m = (uint32_t)(last ? availb : availb - 1);
      if (!reserve(m) || !run_piece(raw, m, last)) return kReadsGaveUp;
      G2S_HIP_TRY_AS(hipEventRecord(done[b].e, cur), (hip_fail(why, what_, e_), kReadsGaveUp));
      used[b] = true;
      info->raw_bytes += n_new;
      have_front = !last;
      halo_at = m;
      slot ^= 1;
      if (last) break;
    }
    have_front = false;
    for (int b = 0; b < 2; b++)
      switch (check_window(b)) {
        case kCorrupt: return corrupt("corrupt BGZF member");
        case kRefused: return kReadsGaveUp;
        default: break;
      }
    *how = used_dev ? (used_zlib ? kInflateMixed : kInflateDevice) : used_zlib ? kInflateZlib : kInflateNone;
    return kReadsOk;
  }
};

}  // namespace

ReadsLoadResult load_reads_device(const std::vector<ReadsInput>& inputs, int device, size_t piece, uint64_t first_cap,
                                  bool host_inflate, DeviceText* out, ReadsLoadInfo* info, std::string* err,
                                  uint64_t resident_cap, int bam_stream, bool device_gzip) {
  *info = ReadsLoadInfo();
  if (!filter_device_usable(device)) { *err = "no usable gfx950 device " + std::to_string(device); return kReadsGaveUp; }
  // the text's bound: an uncompressed file gives no more text than it has bytes; compressed input has no bound
  uint64_t plain = 0;
  bool bounded = true;
  for (const ReadsInput& in : inputs) {
    // (a BAM file's text is sized from its count when its turn comes: it adds nothing to the first capacity)
    if (in.mem || in.path.empty()) {
      if (is_bam(in.mem, in.mem_n)) continue;
      plain += in.mem_n;
      bounded = bounded && !is_gzip(in.mem, in.mem_n);
      continue;
    }
    // (stat before any open: a FIFO, /dev/stdin or a process substitution is the host loader's to read, once, from its
    // first byte — opening and closing it here would break its writer)
    struct stat st;
    uint8_t magic[2] = {0, 0};
    if (::stat(in.path.c_str(), &st) != 0) { *err = "cannot read " + in.path; return kReadsIoError; }
    if (!S_ISREG(st.st_mode)) { *err = in.path + " is not a regular file"; return kReadsGaveUp; }
    const int fd = ::open(in.path.c_str(), O_RDONLY);
    if (fd < 0) { *err = "cannot read " + in.path; return kReadsIoError; }
    const ssize_t got = pread(fd, magic, 2, 0);
    bool bam = false;
    if (got == 2 && is_gzip(magic, 2)) {  // (the head of the file: a BAM file says so in its first members)
      std::vector<uint8_t> head((size_t)std::min<uint64_t>((uint64_t)st.st_size, (uint64_t)1 << 18));
      const ssize_t h = pread(fd, head.data(), head.size(), 0);
      bam = h > 0 && is_bam(head.data(), (size_t)h);
    }
    ::close(fd);
    if (bam) continue;
    plain += (uint64_t)st.st_size;
    bounded = bounded && !(got == 2 && is_gzip(magic, 2));
  }
  Loader L;
  L.device = device;
  // (piece 0: a quarter of the raw bytes expected, so that reading overlaps the copies and kernels, within 1 - 32 MiB:
  // the two page-locked buffers cost their size to make, which a small file would pay for nothing)
  const uint64_t expect = bounded ? plain : 4 * plain;
  L.piece = piece ? std::max<size_t>(piece, 16)
                  : (size_t)std::min<uint64_t>((uint64_t)32 << 20, std::max<uint64_t>((uint64_t)1 << 20, (expect / 4 + 65535) & ~(uint64_t)65535));
  L.host_inflate = host_inflate;
  L.bam_window = piece;
  L.resident_cap = resident_cap;
  L.bam_stream = bam_stream;
  L.device_gzip = device_gzip;
  L.info = info;
  L.why = err;
  // (compressed reads: four times their bytes to begin with, and from there by doubling)
  const uint64_t cap0 = bounded ? device_text_bytes(plain) : first_cap ? first_cap : device_text_bytes(4 * plain);
  size_t free_b = 0, total_b = 0;
  if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) { *err = "the device cannot be used"; return kReadsGaveUp; }
  if ((double)cap0 > 0.5 * (double)free_b) { *err = "the text does not fit on the device"; return kReadsGaveUp; }
  L.mem_limit = std::min<uint64_t>(free_b / 2, resident_cap ? resident_cap : UINT64_MAX);
  const bool debug = getenv("G2S_DEBUG") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  if (!L.init(cap0)) return kReadsGaveUp;
  const auto t1 = std::chrono::steady_clock::now();
  for (const ReadsInput& in : inputs) {
    int how = kInflateNone;
    const ReadsLoadResult r = L.run_file(in, &how);
    if (r == kReadsIoError) { *err = L.io_error; return r; }
    if (r != kReadsOk) return r;
    info->inflate.push_back(how);
    info->files++;
  }
  FxCarry c;
  if (!L.read_carry(&c)) return kReadsGaveUp;
  if (c.overflow) { *err = "the text outgrew its bound"; return kReadsGaveUp; }
  const uint64_t T = c.base, need = device_text_bytes(T);
  if (need > L.cap && !L.grow(need, T)) return kReadsGaveUp;
  hipLaunchKernelGGL(k_fastx_fill, dim3(256), dim3(256), 0, L.cur, L.d_text.as<uint8_t>() + T, need - T, (uint8_t)'N');
  if (hipStreamSynchronize(L.cur) != hipSuccess || hipGetLastError() != hipSuccess) { *err = "the device refused the text's padding"; return kReadsGaveUp; }
  if (debug)
    fprintf(stderr, "[g2s]   reads on the device: buffers %.1f ms, files %.1f ms (pieces of %zu bytes)\n",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(), L.piece);
  info->positions = T;
  info->records = c.records;
  info->on_device = 1;
  info->bam_kernels = info->bam_files && !L.bam_by_host ? 1 : 0;
  info->bam_reason = info->bam_kernels ? kBamReadsKernels : kBamReadsNotAsked;
  out->d_text = (uint8_t*)L.d_text.release();
  out->T = T;
  out->capacity = L.cap;
  out->device = device;
  return kReadsOk;
}

}  // namespace g2s
