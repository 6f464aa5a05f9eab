// gap2seq_amd/csrc/bgzf_inflate.hip — BGZF members inflated on the GPU: g2s_bgzf_inflate, and the buffers of a window
// on its way through the device (bgzf_inflate.h).
//
// One wave a member, one member a workgroup.  The decoder is inflate_core.h: its bit buffer, its table look-ups and
// every branch are the same in all 64 lanes (the look-ups are read through G2S_INF_UNIFORM), so one symbol after another
// is decoded by the wave as by one thread; the lanes work together where bytes move:
//   literals       the wave keeps up to 64 pending literals, lane i the i-th, and stores them with one instruction
//   a match        lane i copies byte i, i + 64, ... of the match from (i mod distance) bytes behind the match's source:
//                  every byte read lies in front of the match, so the overlapping case (distance < length, periodic with
//                  period `distance`) needs no order among the lanes
//   stored blocks  the lanes copy the bytes from the input
// Layout kept: the WHOLE member in LDS (64 KiB + 16) beside the decode tables (4.1 KiB) and the CRC byte table (1 KiB),
// 70.2 KiB a workgroup, two members a CU out of 160 KiB.  Every back-reference is then an LDS read whatever its
// distance, and the member leaves for HBM once, behind its CRC check, as words by all lanes.  (A 32 KiB sliding window
// with four members a CU was not built: it was not measured)
//   CRC-32         lane i computes the CRC of the member's i-th slice (inflate_core.h: crc_slice_bytes) from LDS with the
//                  byte table, multiplies it by x^(8 * bytes behind the slice) mod P, and the wave XORs the 64 products.
// A member's status word says what happened to it; nothing is written for a member that is not kOk.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bgzf_inflate.h"
#include "hip_host.h"
#include "inflate_core.h"
#include "readfilter_gaps.hpp"

namespace {

namespace inf = g2s::inflate;
constexpr uint32_t kWave = 64;

struct WaveSink {
  uint8_t* out;  // the member, in LDS
  uint32_t lane;
  uint32_t lit_at, nlit, mine;  // nlit pending literals for out[lit_at ...]; `mine`: this lane's
  // (a wave's LDS accesses are carried out in the order they were issued: what must not happen is the compiler moving
  // one across the point where another lane's bytes are needed)
  __device__ __forceinline__ void order() { __builtin_amdgcn_wave_barrier(); }
  __device__ __forceinline__ void flush() {
    if (lane < nlit) out[lit_at + lane] = (uint8_t)mine;
    nlit = 0;
    order();
  }
  __device__ __forceinline__ void put(uint32_t at, uint8_t c) {
    if (nlit == 0) lit_at = at;
    if (lane == nlit) mine = c;
    if (++nlit == kWave) flush();
  }
  __device__ __forceinline__ void match(uint32_t at, uint32_t dist, uint32_t len) {
    if (nlit) flush();
    const uint8_t* src = out + (at - dist);
    if (dist >= len) {
      for (uint32_t i = lane; i < len; i += kWave) out[at + i] = src[i];
    } else if (dist == 1) {
      const uint8_t v = src[0];
      for (uint32_t i = lane; i < len; i += kWave) out[at + i] = v;
    } else {
      for (uint32_t i = lane; i < len; i += kWave) out[at + i] = src[i % dist];
    }
    order();
  }
  __device__ __forceinline__ void copy_in(uint32_t at, const uint8_t* from, uint32_t len) {
    if (nlit) flush();
    for (uint32_t i = lane; i < len; i += kWave) out[at + i] = from[i];
    order();
  }
  __device__ __forceinline__ void finish() {
    if (nlit) flush();
  }
};

}  // namespace

__global__ void __launch_bounds__(64) g2s_bgzf_inflate(const uint8_t* __restrict__ comp, const g2s::BgzfMember* __restrict__ mem,
                                                       uint32_t n_members, uint8_t* __restrict__ out,
                                                       uint32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t member_words[inf::kMaxMember / 4 + 4];
  __shared__ uint32_t crc_tab[256];
  __shared__ inf::Tables tables;
  const uint32_t m = blockIdx.x, lane = threadIdx.x;
  if (m >= n_members) return;
  const g2s::BgzfMember d = mem[m];
  uint8_t* member = (uint8_t*)member_words;
  uint32_t st = inf::kOk;
  if (d.isize > inf::kMaxMember) {
    st = inf::kCorrupt;
  } else if (d.isize) {
    for (uint32_t i = lane; i < 256u; i += kWave) crc_tab[i] = inf::crc_table_entry(i);
    WaveSink sink{member, lane, 0, 0, 0};
    st = inf::inflate_member(comp + d.in_off, d.in_len, d.isize, &tables, sink);
    if (st == inf::kOk) {
      __builtin_amdgcn_wave_barrier();
      // ---- the CRC of this lane's slice, moved to its place in the member
      const uint32_t slice = inf::crc_slice_bytes(d.isize);
      const uint32_t lo = lane * slice < d.isize ? lane * slice : d.isize;
      const uint32_t hi = lo + slice < d.isize ? lo + slice : d.isize;
      uint32_t c = 0;
      if (hi > lo) {
        c = 0xFFFFFFFFu;
        for (uint32_t o = lo; o < hi; o += 4u) {  // (lo is a multiple of 4)
          uint32_t w = member_words[o / 4u];
          const uint32_t nb = hi - o < 4u ? hi - o : 4u;
          for (uint32_t k = 0; k < nb; k++, w >>= 8) c = inf::crc_byte(crc_tab, c, (uint8_t)w);
        }
        c = inf::crc_shift(~c, d.isize - hi);
      }
      for (int off = 32; off; off >>= 1) c ^= (uint32_t)__shfl_xor((int)c, off, 64);
      if (c != d.crc) {
        st = inf::kCrcMismatch;
      } else {
        // ---- out: bytes up to the first word boundary of the destination, words, the last bytes
        uint8_t* dst = out + d.out_off;
        const uint32_t head0 = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
        const uint32_t head = head0 < d.isize ? head0 : d.isize;
        const uint32_t words = (d.isize - head) / 4u;
        const uint32_t tail = d.isize - head - 4u * words;
        if (lane < head) dst[lane] = member[lane];
        uint32_t* dw = (uint32_t*)(dst + head);
        if (head == 0) {
          for (uint32_t k = lane; k < words; k += kWave) dw[k] = member_words[k];
        } else {
          const uint32_t sh = 8u * head;
          for (uint32_t k = lane; k < words; k += kWave) dw[k] = member_words[k] >> sh | member_words[k + 1] << (32u - sh);
        }
        if (lane < tail) dst[head + 4u * words + lane] = member[head + 4u * words + lane];
      }
    }
  }
  if (lane == 0) status[m] = st;
}

namespace g2s {

BgzfDevice* BgzfDevice::create(int device, size_t max_in, size_t max_out, size_t max_members, size_t front, std::string* why,
                               bool host_window) {
  if (!filter_device_usable(device)) {
    if (why) *why = "no usable gfx950 device " + std::to_string(device);
    return nullptr;
  }
  BgzfDevice* D = new BgzfDevice();
  D->device_ = device;
  D->front_ = front;
  D->cap_in_ = max_in;
  D->cap_out_ = max_out;
  D->cap_members_ = max_members;
  auto make = [&]() -> bool {
    G2S_HIP_TRY(hipSetDevice(device));
    hipStream_t st;
    G2S_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    D->stream_ = st;
    uint64_t held = 0;  // what the device allocations below ask for
    auto take = [&held](void** p, size_t bytes) {
      held += bytes;
      return hipMalloc(p, bytes);
    };
    for (Slot& s : D->s_) {
      G2S_HIP_TRY(hipHostMalloc((void**)&s.h_in, max_in + 16, hipHostMallocDefault));
      if (host_window) G2S_HIP_TRY(hipHostMalloc((void**)&s.h_out, front + max_out + 16, hipHostMallocDefault));
      G2S_HIP_TRY(hipHostMalloc((void**)&s.h_mem, (max_members + 1) * sizeof(BgzfMember), hipHostMallocDefault));
      G2S_HIP_TRY(hipHostMalloc((void**)&s.h_st, (max_members + 1) * 4, hipHostMallocDefault));
      G2S_HIP_TRY(take((void**)&s.d_in, max_in + 16));
      if (host_window) G2S_HIP_TRY(take((void**)&s.d_out, front + max_out + 64));  // (else: the caller's destination)
      G2S_HIP_TRY(take((void**)&s.d_mem, (max_members + 1) * sizeof(BgzfMember)));
      G2S_HIP_TRY(take((void**)&s.d_st, (max_members + 1) * 4));
      hipEvent_t ev;
      G2S_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      s.done = ev;
    }
    if (held != device_bytes(max_in, max_out, max_members, front, host_window)) {
      if (why) *why = "the slots' allocations are not what device_bytes() says";
      return false;
    }
    return true;
  };
  if (!make()) {
    delete D;
    return nullptr;
  }
  return D;
}

BgzfDevice::~BgzfDevice() {
  if (device_ >= 0) (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
  for (Slot& s : s_) {
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.h_mem) (void)hipHostFree(s.h_mem);
    if (s.h_st) (void)hipHostFree(s.h_st);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.d_mem) (void)hipFree(s.d_mem);
    if (s.d_st) (void)hipFree(s.d_st);
    if (s.done) (void)hipEventDestroy((hipEvent_t)s.done);
  }
  if (stream_) (void)hipStreamDestroy((hipStream_t)stream_);
}

bool BgzfDevice::launch(int slot, size_t n_members, size_t in_bytes, size_t out_bytes, std::string* why, bool down,
                        uint8_t* d_dst) {
  Slot& s = s_[slot];
  hipStream_t st = (hipStream_t)stream_;
  if (!fits(n_members, in_bytes, out_bytes)) {
    if (why) *why = "a window larger than the buffers";
    return false;
  }
  if (!d_dst && !s.d_out) {
    if (why) *why = "a window without a destination";
    return false;
  }
  if (d_dst && down) {
    if (why) *why = "a window with a destination of its own is not copied down";
    return false;
  }
  G2S_HIP_TRY(hipSetDevice(device_));
  if (n_members && out_bytes) {
    if (in_bytes) G2S_HIP_TRY(hipMemcpyAsync(s.d_in, s.h_in, in_bytes, hipMemcpyHostToDevice, st));
    G2S_HIP_TRY(hipMemcpyAsync(s.d_mem, s.h_mem, n_members * sizeof(BgzfMember), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(g2s_bgzf_inflate, dim3((unsigned)n_members), dim3(kWave), 0, st, (const uint8_t*)s.d_in,
                       (const BgzfMember*)s.d_mem, (uint32_t)n_members, d_dst ? d_dst : s.d_out + front_, s.d_st);
    G2S_HIP_TRY(hipGetLastError());
    if (down) G2S_HIP_TRY(hipMemcpyAsync(s.h_out + front_, s.d_out + front_, out_bytes, hipMemcpyDeviceToHost, st));
    G2S_HIP_TRY(hipMemcpyAsync(s.h_st, s.d_st, n_members * 4, hipMemcpyDeviceToHost, st));
  } else {
    memset(s.h_st, 0, n_members * 4);  // (members without bytes succeed: inflate_core.h kOk)
  }
  G2S_HIP_TRY(hipEventRecord((hipEvent_t)s.done, st));
  s.busy = true;
  return true;
}

bool BgzfDevice::wait(int slot, std::string* why) {
  Slot& s = s_[slot];
  if (!s.busy) return true;
  s.busy = false;
  G2S_HIP_TRY(hipSetDevice(device_));
  G2S_HIP_TRY(hipEventSynchronize((hipEvent_t)s.done));
  return true;
}

}  // namespace g2s
