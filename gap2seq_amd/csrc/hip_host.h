// gap2seq_amd/csrc/hip_host.h — the host side's plumbing around HIP and rocPRIM, once, for the .hip files of the graph
// build and the read filter (dbg_gpu, readfilter_gpu, bam_rows, bam_store, bam_text, bgzf_inflate, seg_tables): an owned device
// allocation, page-locked buffer and event, "run this HIP call or leave with its text", rocPRIM's two-call protocol, scan-and-total, "is there such a
// device".  Host only; no kernel, no other project header.  (g2s_api.hip's DevBuf / PinBuf are grow-only session buffers,
// another thing.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>  // (rocprim.hpp calls memset and includes nothing that declares it)
#include <string>

#include <rocprim/rocprim.hpp>

namespace g2s {

// ---- an owned device allocation.  Members and locals free themselves in reverse order of declaration; free() is for the
// places where memory has to go early (the peak-memory comments at the call sites).
struct DevMem {
  void* p = nullptr;
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.release()) {}
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) { free(); p = o.release(); }
    return *this;
  }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { free(); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }  // (never a null pointer for no bytes)
  void free() { if (p) (void)hipFree(release()); }
  void* release() { void* q = p; p = nullptr; return q; }  // the caller owns it from here (DeviceGraph's kept tables)
  template <class T> T* as() const { return (T*)p; }
};

// ---- an owned page-locked host allocation (a staging buffer of an asynchronous copy) and an owned event
struct PinMem {
  void* p = nullptr;
  PinMem() = default;
  PinMem(const PinMem&) = delete;
  PinMem& operator=(const PinMem&) = delete;
  ~PinMem() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault); }
};
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  ~DevEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
};

// ---- "<expression>: <error string>", and the ways to leave with it
inline std::string hip_message(const char* what, hipError_t e) { return std::string(what) + ": " + hipGetErrorString(e); }
inline bool hip_fail(std::string* why, const char* what, hipError_t e) {
  if (why) *why = hip_message(what, e);
  return false;
}
// the general form: `result` is what the function returns, and may name what_ (the expression's text) and e_
#define G2S_HIP_TRY_AS(expr, result)                 \
  do {                                               \
    const hipError_t e_ = (expr);                    \
    if (e_ != hipSuccess) {                          \
      const char* what_ = #expr;                     \
      return result;                                 \
    }                                                \
  } while (0)
// in a function that returns false with `std::string* why` (may be null) set
#define G2S_HIP_TRY(expr) G2S_HIP_TRY_AS(expr, ::g2s::hip_fail(why, what_, e_))
// in a function that returns a code of the C ABI with `std::string* err` set.  The header knows no code of the ABI: the
// file that uses this form defines `int hip_code(hipError_t)`, the code an error leaves with (readfilter_gpu.hip)
#define G2S_HIP_TRY_CODE(expr) G2S_HIP_TRY_AS(expr, (*err = ::g2s::hip_message(what_, e_), hip_code(e_)))

inline bool device_exists(int device) {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev;
}

// ---- rocPRIM: size query, scratch, run.  A Scratch that is empty is sized and allocated by the first call it is given
// to and serves the calls after it; p / bytes set by hand make it a piece of the caller's own memory (bam_text.hip's
// arena).  Every call is handed the Scratch's true size, and rocPRIM compares it with what the call needs: one that needs
// more fails with hipErrorInvalidValue and writes nothing.  The forms without a Scratch use one of their own.
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  DevMem own;
  void free() { own.free(); p = nullptr; bytes = 0; }
};

namespace detail {
template <class F> hipError_t prim_reserve(Scratch& s, F&& call) {
  hipError_t e = call(nullptr, s.bytes);
  if (e == hipSuccess && (e = s.own.alloc(s.bytes)) == hipSuccess) s.p = s.own.p;
  return e;
}
template <class F> hipError_t prim_run(Scratch& s, F&& call) {
  if (!s.p) {
    const hipError_t e = prim_reserve(s, call);
    if (e != hipSuccess) return e;
  }
  size_t bytes = s.bytes;  // (the calls take the size by reference)
  return call(s.p, bytes);
}
}  // namespace detail

// out[i] = in[0] + ... + in[i - 1]
template <class In, class T> hipError_t exclusive_scan(Scratch& s, In in, T* out, size_t n, hipStream_t st = 0) {
  return detail::prim_run(s, [&](void* tmp, size_t& b) { return rocprim::exclusive_scan(tmp, b, in, out, (T)0, n, rocprim::plus<T>(), st); });
}
template <class In, class T> hipError_t exclusive_scan(In in, T* out, size_t n) {
  Scratch s;
  return exclusive_scan(s, in, out, n);
}
// the bytes a scan of n T's wants (a size query reads no array)
template <class T> hipError_t exclusive_scan_bytes(size_t n, size_t* bytes, hipStream_t st = 0) {
  return rocprim::exclusive_scan(nullptr, *bytes, (T*)nullptr, (T*)nullptr, (T)0, n, rocprim::plus<T>(), st);
}
// the sum of all n >= 1 inputs behind their scan: the last input plus the last output, two blocking copies
template <class In, class T> hipError_t read_total(In in, const T* out, size_t n, T* total) {
  T last_in = 0, last_out = 0;
  hipError_t e = hipMemcpy(&last_in, in + (n - 1), sizeof(T), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&last_out, out + (n - 1), sizeof(T), hipMemcpyDeviceToHost);
  *total = last_in + last_out;
  return e;
}
template <class In, class T> hipError_t scan_total(Scratch& s, In in, T* out, size_t n, T* total) {
  const hipError_t e = exclusive_scan(s, in, out, n);
  return e == hipSuccess ? read_total(in, out, n, total) : e;
}
template <class In, class T> hipError_t scan_total(In in, T* out, size_t n, T* total) {
  Scratch s;
  return scan_total(s, in, out, n, total);
}

// ascending, stable, on bits [0, end_bit) of the keys
template <class KIn, class K> hipError_t radix_sort_keys(Scratch& s, KIn in, K* out, size_t n, unsigned end_bit = 8 * sizeof(K)) {
  return detail::prim_run(s, [&](void* tmp, size_t& b) { return rocprim::radix_sort_keys(tmp, b, in, out, n, 0, end_bit); });
}
template <class KIn, class K, class VIn, class V>
hipError_t radix_sort_pairs(Scratch& s, KIn kin, K* kout, VIn vin, V* vout, size_t n, unsigned end_bit = 8 * sizeof(K)) {
  return detail::prim_run(s, [&](void* tmp, size_t& b) { return rocprim::radix_sort_pairs(tmp, b, kin, kout, vin, vout, n, 0, end_bit); });
}
// the scratch of the full-width pair sorts of n items that follow, taken before the first of them
template <class K, class V> hipError_t radix_sort_pairs_reserve(Scratch& s, size_t n) {
  return detail::prim_reserve(s, [&](void* tmp, size_t& b) {
    return rocprim::radix_sort_pairs(tmp, b, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, n, 0, 8 * sizeof(K));
  });
}
// the first of every run of equal items; *count (device memory) = how many
template <class In, class T> hipError_t unique(Scratch& s, In in, T* out, uint64_t* count, size_t n) {
  return detail::prim_run(s, [&](void* tmp, size_t& b) { return rocprim::unique(tmp, b, in, out, count, n); });
}

}  // namespace g2s
