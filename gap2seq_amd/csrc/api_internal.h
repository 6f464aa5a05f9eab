// gap2seq_amd/csrc/api_internal.h — what the units of the C ABI share (g2s_api.hip, api_graph.hip, api_test_hooks.hip):
// the error macros, wall time, the graph handle and the functions one unit calls in another.  Nothing here is
// exported: the library's interface is include/g2s.h.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "../../include/g2s.h"
#include "../../include/g2s_test.h"
#include "dbg.hpp"
#include "envcache.hpp"

#pragma GCC visibility push(hidden)

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(G2S_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)
// (resident mode: kernels of the list may be in flight on the session's streams and write the caller's pinned buffers
// — an error return waits for them first)
#define HIP_TRY_S(expr)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (void)hipStreamSynchronize(s->stream);                                                  \
      (void)hipStreamSynchronize(s->stream2);                                                 \
      if (s->stream3) (void)hipStreamSynchronize(s->stream3);                                 \
      return fail(G2S_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    }                                                                                         \
  } while (0)

// wall time in milliseconds: between two time points, and from one until now
using TimePoint = std::chrono::steady_clock::time_point;
static inline double ms_between(TimePoint a, TimePoint b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static inline double ms_since(TimePoint t0) { return ms_between(t0, std::chrono::steady_clock::now()); }

struct g2s_graph {
  g2s::Graph* g = nullptr;
};

// the functions one unit calls in another, both of g2s_api.hip (fail() writes the calling thread's error text, which
// is private to that unit; g2s_last_error() reads it)
namespace g2s {
namespace api {
int fail(int code, const std::string& msg);
int ensure_seg_tables(g2s_graph* g, int device);
}  // namespace api
}  // namespace g2s

#pragma GCC visibility pop
