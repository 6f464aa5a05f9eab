// gap2seq_amd/csrc/bam_text.hip — pass B of the batched read filter on the GPU (bam_text.h): from the inflated stream
// pass A left in device memory to the bases, names and FASTA text of the selected records, without a second inflate
// and without the host walking a record.
//
//   lengths   k_lengths   one thread a row reads l_name, the flag and l_seq from the record's head at its offset and the
//                         name's length up to its first NUL, and gives the bytes the row adds to each of the two
//                         outputs, A and B (pool form: bases and name; text form: the row's FASTA record in the
//                         selected text and in the unmapped text), whether it is held and whether it is an unmapped
//                         read that is wanted.  It checks the record's layout against the stream's end once more.
//   offsets               four exclusive scans (rocPRIM) over n + 1 entries: where every row's bytes go, its index among
//                         the held ones, its index among the unmapped ones; entry n holds the totals, which size every
//                         output before it is written (k_totals gathers them for one copy down).
//   entries   k_entries   pool form: base_off / name_off per held record, the unmapped list, the index by row
//                         (BamTextAsk::device_text: a held record's bases count one byte more, the 'N' k_decode writes
//                         behind them, so that base_off is the read's start in the pooled build's text; that text and
//                         the starts go into an allocation of their own, which the caller keeps, and nothing of
//                         either output comes down but the offsets)
//   decode    k_decode    a wave a row, the lanes over the row's output bytes, 64 consecutive bytes a step, so that a
//                         wave's store is one run of bytes whatever the read's length.  A wave takes 64 rows at a time,
//                         finds the ones with output by ballot and visits those alone.
// Every index is checked against its array's size before a write; a record that does not lie within the stream sets a
// flag that fails the call (the caller then takes the host route).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bam.hpp"
#include "bam_decode.h"
#include "bam_text.h"
#include "device_pool.h"
#include "hip_host.h"

namespace {

using namespace g2s::bam_decode;  // (kWave, kRecHead, ld32, Piece, emit: one record's bytes by a wave)

constexpr uint32_t kBlock = 256;

// what comes down between the scans and the outputs, in one copy
struct Totals {
  uint32_t bad;  // a record outside the stream, or a layout outside its block_size
  uint32_t n_held, n_un, pad_;
  uint64_t bytes_a, bytes_b;
};

// (n + 1 entries each: entry n is 0, so that the scans' entry n is the total)
__global__ void __launch_bounds__(kBlock) k_lengths(const uint8_t* __restrict__ stream, uint64_t stream_bytes,
                                                    const uint64_t* __restrict__ rec_off, uint64_t n,
                                                    const uint8_t* __restrict__ sel, int pool, int names, int unmapped,
                                                    uint64_t* __restrict__ len_a, uint64_t* __restrict__ len_b,
                                                    uint32_t* __restrict__ held, uint32_t* __restrict__ un, Totals* tot) {
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  uint64_t a = 0, b = 0;
  uint32_t h = 0, u = 0;
  if (r < n) {
    const uint64_t off = rec_off[r];
    bool ok = off + kRecHead <= stream_bytes;
    if (ok) {
      const uint8_t* rec = stream + off;
      const uint32_t bs = ld32(rec), l_name = rec[12], w = ld32(rec + 16), n_cigar = w & 0xFFFFu, flag = w >> 16;
      const int32_t l_seq = (int32_t)ld32(rec + 20);
      ok = l_seq >= 0 && l_name != 0 && off + 4 + (uint64_t)bs <= stream_bytes &&
           32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 <= bs;
      if (ok) {
        const bool is_un = unmapped && (flag & g2s::BAM_UNMAPPED), chosen = sel[r] != 0;
        if (chosen || is_un) {
          const uint8_t* name = rec + kRecHead;
          uint32_t nl = 0;
          while (nl < l_name && name[nl]) nl++;
          if (pool) {
            h = 1;
            u = is_un ? 1u : 0u;
            a = (uint64_t)l_seq + (pool == 2 ? 1u : 0u);  // (2: the build's layout, an 'N' behind every read)
            b = names ? nl + 2u : 0u;
          } else {
            const uint64_t fasta = (uint64_t)nl + 5u + (uint64_t)l_seq;  // > name /1 \n bases \n
            a = chosen ? fasta : 0;
            b = is_un ? fasta : 0;
            h = chosen ? 1u : 0u;
            u = is_un ? 1u : 0u;
          }
        }
      }
    }
    if (!ok) tot->bad = 1;
  }
  len_a[r] = a;
  len_b[r] = b;
  held[r] = h;
  un[r] = u;
}

__global__ void __launch_bounds__(kBlock) k_entries(uint64_t n, const uint32_t* __restrict__ held, const uint32_t* __restrict__ un,
                                                    const uint64_t* __restrict__ off_a, const uint64_t* __restrict__ off_b,
                                                    const uint32_t* __restrict__ idx, const uint32_t* __restrict__ uidx,
                                                    uint64_t n_held, uint64_t n_un, uint64_t* __restrict__ base_off,
                                                    uint64_t* __restrict__ name_off, uint32_t* __restrict__ unmapped_read,
                                                    uint32_t* __restrict__ pidx) {
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r > n) return;
  if (r == n) {  // (the closing offsets)
    base_off[n_held] = off_a[n];
    name_off[n_held] = off_b[n];
    return;
  }
  const uint32_t i = idx[r];
  if (held[r] && i < n_held) {
    base_off[i] = off_a[r];
    name_off[i] = off_b[r];
    pidx[r] = i;
    if (un[r] && uidx[r] < n_un) unmapped_read[uidx[r]] = i;
  } else {
    pidx[r] = 0;
  }
}

// entry n of the four scans, beside the flag k_lengths set
__global__ void k_totals(uint64_t n, const uint64_t* __restrict__ off_a, const uint64_t* __restrict__ off_b,
                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ uidx, Totals* tot) {
  tot->bytes_a = off_a[n];
  tot->bytes_b = off_b[n];
  tot->n_held = idx[n];
  tot->n_un = uidx[n];
}

template <int PIECE_A, int PIECE_B>
__global__ void __launch_bounds__(kBlock) k_decode(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ rec_off,
                                                   uint64_t n, const uint64_t* __restrict__ off_a,
                                                   const uint64_t* __restrict__ off_b, uint8_t* __restrict__ out_a,
                                                   uint64_t cap_a, uint8_t* __restrict__ out_b, uint64_t cap_b) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t chunks = (n + kWave - 1) / kWave;
  for (uint64_t c = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave; c < chunks; c += waves) {
    const uint64_t mine = c * kWave + lane;
    const bool some = mine < n && (off_a[mine + 1] != off_a[mine] || off_b[mine + 1] != off_b[mine]);
    uint64_t mask = __ballot(some);
    while (mask) {
      const uint64_t r = c * kWave + (uint64_t)__builtin_ctzll(mask);
      mask &= mask - 1;
      const uint8_t* rec = stream + rec_off[r];
      const uint64_t a0 = off_a[r], a1 = off_a[r + 1], b0 = off_b[r], b1 = off_b[r + 1];
      if (a1 > a0 && a1 <= cap_a) emit<PIECE_A>(rec, a1 - a0, out_a + a0, lane);
      if (b1 > b0 && b1 <= cap_b) emit<PIECE_B>(rec, b1 - b0, out_b + b0, lane);
    }
  }
}

// a piece of an Arena
struct Buf {
  void* p = nullptr;
  template <class T> T* as() const { return (T*)p; }
};
// one device allocation cut into pieces of 256-byte alignment (an allocation and its release cost more than the kernels
// here): add() every piece, get(), then the pieces point into it
struct Arena {
  g2s::DevMem base;
  size_t bytes = 0;
  std::vector<std::pair<Buf*, size_t>> pieces;
  void add(Buf* b, size_t n) {
    pieces.push_back({b, bytes});
    bytes += (n + 255) & ~(size_t)255;
  }
  hipError_t get() {
    const hipError_t e = base.alloc(bytes ? bytes : 256);
    if (e == hipSuccess)
      for (auto& pc : pieces) pc.first->p = base.as<uint8_t>() + pc.second;
    return e;
  }
};

}  // namespace

namespace g2s {

bool bam_text_device(const BamRowsDevice& rows, const uint8_t* sel, const BamTextAsk& ask, BamText* out, std::string* why) {
  const DeviceRows& R = rows.rows();
  const uint64_t n = R.n;
  if (!rows.stream_buffer() || !R.rec_off) {
    if (why) *why = "no resident stream";
    return false;
  }
  *out = BamText();
  if (ask.pool) out->pidx.assign((size_t)n, 0);
  else { out->toff.assign((size_t)n, 0); out->tlen.assign((size_t)n, 0); }
  if (!n) return true;
  hipStream_t s = (hipStream_t)rows.stream();
  G2S_HIP_TRY(hipSetDevice(rows.device()));
  const bool device_text = ask.pool && ask.device_text;
  const size_t m = (size_t)n + 1;
  const unsigned groups = (unsigned)((m + kBlock - 1) / kBlock);
  Buf d_sel, d_len_a, d_len_b, d_held, d_un, d_off_a, d_off_b, d_idx, d_uidx, d_tot, d_tmp;
  size_t tb64 = 0, tb32 = 0;
  G2S_HIP_TRY(exclusive_scan_bytes<uint64_t>(m, &tb64, s));
  G2S_HIP_TRY(exclusive_scan_bytes<uint32_t>(m, &tb32, s));
  const size_t tb = tb64 > tb32 ? tb64 : tb32;
  Arena work;
  work.add(&d_sel, (size_t)n);
  work.add(&d_len_a, m * 8);
  work.add(&d_len_b, m * 8);
  work.add(&d_held, m * 4);
  work.add(&d_un, m * 4);
  work.add(&d_off_a, m * 8);
  work.add(&d_off_b, m * 8);
  work.add(&d_idx, m * 4);
  work.add(&d_uidx, m * 4);
  work.add(&d_tot, sizeof(Totals));
  work.add(&d_tmp, tb);
  G2S_HIP_TRY(work.get());
  G2S_HIP_TRY(hipMemcpyAsync(d_sel.p, sel, (size_t)n, hipMemcpyHostToDevice, s));
  G2S_HIP_TRY(hipMemsetAsync(d_tot.p, 0, sizeof(Totals), s));
  hipLaunchKernelGGL(k_lengths, dim3(groups), dim3(kBlock), 0, s, (const uint8_t*)rows.stream_buffer(), rows.stream_bytes(),
                     (const uint64_t*)R.rec_off, n, d_sel.as<const uint8_t>(), ask.pool ? (device_text ? 2 : 1) : 0, (int)ask.names, (int)ask.unmapped,
                     d_len_a.as<uint64_t>(), d_len_b.as<uint64_t>(), d_held.as<uint32_t>(), d_un.as<uint32_t>(), d_tot.as<Totals>());
  G2S_HIP_TRY(hipGetLastError());
  // ---- the offsets
  Scratch tmp;  // (the arena's piece serves all four)
  tmp.p = d_tmp.p;
  tmp.bytes = tb;
  G2S_HIP_TRY(exclusive_scan(tmp, d_len_a.as<uint64_t>(), d_off_a.as<uint64_t>(), m, s));
  G2S_HIP_TRY(exclusive_scan(tmp, d_len_b.as<uint64_t>(), d_off_b.as<uint64_t>(), m, s));
  G2S_HIP_TRY(exclusive_scan(tmp, d_held.as<uint32_t>(), d_idx.as<uint32_t>(), m, s));
  G2S_HIP_TRY(exclusive_scan(tmp, d_un.as<uint32_t>(), d_uidx.as<uint32_t>(), m, s));
  hipLaunchKernelGGL(k_totals, dim3(1), dim3(1), 0, s, n, d_off_a.as<const uint64_t>(), d_off_b.as<const uint64_t>(),
                     d_idx.as<const uint32_t>(), d_uidx.as<const uint32_t>(), d_tot.as<Totals>());
  G2S_HIP_TRY(hipGetLastError());
  Totals tot{};
  G2S_HIP_TRY(hipMemcpyAsync(&tot, d_tot.p, sizeof tot, hipMemcpyDeviceToHost, s));
  G2S_HIP_TRY(hipStreamSynchronize(s));
  const uint64_t bytes_a = tot.bytes_a, bytes_b = tot.bytes_b;
  const uint32_t n_held = tot.n_held, n_un = tot.n_un;
  if (tot.bad) {
    if (why) *why = "a record outside the resident stream";
    return false;
  }
  // ---- the outputs, sized by their counts
  Buf d_out_a, d_out_b, d_boff, d_noff, d_unl, d_pidx;
  Arena outs, keep;  // (keep: what a device_text caller takes over)
  (device_text ? keep : outs).add(&d_out_a, (size_t)bytes_a);
  outs.add(&d_out_b, device_text ? 0 : (size_t)bytes_b);
  if (ask.pool) {
    (device_text ? keep : outs).add(&d_boff, ((size_t)n_held + 1) * 8);
    outs.add(&d_noff, ((size_t)n_held + 1) * 8);
    outs.add(&d_unl, (size_t)n_un * 4);
    outs.add(&d_pidx, (size_t)n * 4);
  }
  G2S_HIP_TRY(outs.get());
  if (device_text) G2S_HIP_TRY(keep.get());
  const unsigned waves_wanted = (unsigned)((n + kWave - 1) / kWave);
  const unsigned dgroups = std::max(1u, std::min((waves_wanted + kBlock / kWave - 1) / (kBlock / kWave), 256u * 16u));
  if (ask.pool) {
    hipLaunchKernelGGL(k_entries, dim3(groups), dim3(kBlock), 0, s, n, d_held.as<const uint32_t>(), d_un.as<const uint32_t>(),
                       d_off_a.as<const uint64_t>(), d_off_b.as<const uint64_t>(), d_idx.as<const uint32_t>(),
                       d_uidx.as<const uint32_t>(), (uint64_t)n_held, (uint64_t)n_un, d_boff.as<uint64_t>(), d_noff.as<uint64_t>(),
                       d_unl.as<uint32_t>(), d_pidx.as<uint32_t>());
    hipLaunchKernelGGL((k_decode<kBases, kName>), dim3(dgroups), dim3(kBlock), 0, s, (const uint8_t*)rows.stream_buffer(),
                       (const uint64_t*)R.rec_off, n, d_off_a.as<const uint64_t>(), d_off_b.as<const uint64_t>(),
                       d_out_a.as<uint8_t>(), bytes_a, d_out_b.as<uint8_t>(), device_text ? 0 : bytes_b);  // (cap 0: no names)
  } else {
    hipLaunchKernelGGL((k_decode<kFasta, kFasta>), dim3(dgroups), dim3(kBlock), 0, s, (const uint8_t*)rows.stream_buffer(),
                       (const uint64_t*)R.rec_off, n, d_off_a.as<const uint64_t>(), d_off_b.as<const uint64_t>(),
                       d_out_a.as<uint8_t>(), bytes_a, d_out_b.as<uint8_t>(), bytes_b);
  }
  G2S_HIP_TRY(hipGetLastError());
  // ---- down, once
  if (ask.pool) {
    if (!device_text) out->pbases.resize((size_t)bytes_a);
    out->pboff.assign((size_t)n_held + 1, 0);
    out->punmapped.assign((size_t)n_un, 0);
    if (bytes_a && !device_text) G2S_HIP_TRY(hipMemcpyAsync(&out->pbases[0], d_out_a.p, (size_t)bytes_a, hipMemcpyDeviceToHost, s));
    G2S_HIP_TRY(hipMemcpyAsync(out->pboff.data(), d_boff.p, ((size_t)n_held + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_un) G2S_HIP_TRY(hipMemcpyAsync(out->punmapped.data(), d_unl.p, (size_t)n_un * 4, hipMemcpyDeviceToHost, s));
    G2S_HIP_TRY(hipMemcpyAsync(out->pidx.data(), d_pidx.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (ask.names) {
      if (!device_text) out->pnames.resize((size_t)bytes_b);
      out->pnoff.assign((size_t)n_held + 1, 0);
      if (bytes_b && !device_text) G2S_HIP_TRY(hipMemcpyAsync(&out->pnames[0], d_out_b.p, (size_t)bytes_b, hipMemcpyDeviceToHost, s));
      G2S_HIP_TRY(hipMemcpyAsync(out->pnoff.data(), d_noff.p, ((size_t)n_held + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    G2S_HIP_TRY(hipStreamSynchronize(s));  // (a device_text caller reads the text from other streams from here on)
    if (device_text) {
      for (size_t i = 0; i <= (size_t)n_held; i++) out->pboff[i] -= i;  // (the starts without the separators in front)
      out->d_start = d_boff.as<const uint64_t>();
      out->d_bytes = keep.bytes;
      out->d_device = rows.device();
      out->d_text = keep.base.release();
    }
  } else {
    std::vector<uint64_t> off(m);
    out->text.resize((size_t)bytes_a);
    out->unmapped.resize((size_t)bytes_b);
    if (bytes_a) G2S_HIP_TRY(hipMemcpyAsync(&out->text[0], d_out_a.p, (size_t)bytes_a, hipMemcpyDeviceToHost, s));
    if (bytes_b) G2S_HIP_TRY(hipMemcpyAsync(&out->unmapped[0], d_out_b.p, (size_t)bytes_b, hipMemcpyDeviceToHost, s));
    G2S_HIP_TRY(hipMemcpyAsync(off.data(), d_off_a.p, m * 8, hipMemcpyDeviceToHost, s));
    G2S_HIP_TRY(hipStreamSynchronize(s));
    for (size_t r = 0; r < (size_t)n; r++)
      if (sel[r]) {  // (a row nothing selected keeps offset and length 0, as on the host walk)
        out->toff[r] = off[r];
        out->tlen[r] = (uint32_t)(off[r + 1] - off[r]);
      }
    out->n_unmapped = (int64_t)n_un;
  }
  return true;
}

void device_pool_release(int device, void* p) {
  if (!p) return;
  (void)hipSetDevice(device);
  (void)hipFree(p);
}

bool device_pool_copy_down(int device, const void* d_text, uint64_t off, uint64_t n, void* dst, std::string* why) {
  if (!n) return true;
  G2S_HIP_TRY(hipSetDevice(device));
  G2S_HIP_TRY(hipMemcpy(dst, (const uint8_t*)d_text + off, (size_t)n, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace g2s
