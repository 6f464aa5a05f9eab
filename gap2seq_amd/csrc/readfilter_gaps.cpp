// gap2seq_amd/csrc/readfilter_gaps.cpp — g2s_filter_reads_gaps: the reads of N gaps from one library in two
// inflating passes over the BAM, whatever N is.  Gap i's outputs are g2s_filter_reads' for gap i, byte for byte.
//
//   pass A (device kernels or host walk)  one compact row per record (readfilter_gaps.hpp: FilterRows): reference, position,
//                                     end position, flag, std::hash of the read's name and of its mate's.  The record
//                                     count and the longest read fall out of it, so every gap's windows are known at
//                                     its end.
//   joins (device or host threads)    per gap the filter's bits (B_g), list 1 (records whose mate's bit is in B_g) and
//                                     list 2 (records overlapping the flanks whose own bit is not), as (gap, row) pairs
//                                     in (gap, row) order: readfilter_gpu.hip, or filter_join_host below.
//   pass B (host walk, or device      the FASTA text of every row some gap (or the unmapped list) selected; every gap's
//           kernels in one-pass mode) text is its list 1 rows' text followed by its list 2 rows'.
//
// With device inflate pass A's rows can be made by kernels from the inflated windows where they lie (bam_rows.hip:
// G2S_DEVICE_ROWS=1 / G2S_HOST_ROWS=1, kDeviceRowsDefault), and the joins read them there; whatever those kernels cannot
// account for hands pass A to the host walk, which is the authority on a file's errors.
// Both passes read the file through BamFile (bam.cpp), which inflates it on the device the joins run on
// (bgzf_inflate.hip, a window ahead of the walk) or with zlib on host threads (no device, G2S_HOST_INFLATE=1).
// By default pass B is a second walk of the host over the file, inflated a second time rather than keeping every
// record's bases from pass A on the host (which would save that inflate and cost half a byte of every base of the file
// there): the host holds 36 bytes a record (the rows), then 13 bytes a record (pass B's selection and text offsets) and
// the text of the SELECTED records, once each however many gaps select them.  The per-gap outputs themselves are the
// text of each gap's reads.
// One-pass mode (g2s_filter_set_one_pass, G2S_FILTER_ONE_PASS=1; off unless asked for): when the joins, the inflate and
// pass A's rows all run on the device and the inflated file fits half the free device memory with the rows
// (G2S_FILTER_RESIDENT_CAP lowers that), pass A inflates every window to its place in one device allocation and
// records every row's offset in it, and pass B is kernels (bam_text.hip) that gather and decode the selected records
// from there: the file is inflated once and the host walks nothing.  Whatever stands in the way — not asked for, no
// device rows, over the cap, a failed allocation or HIP call — sends the call down the two-pass route from the point it
// is at, with the resident buffer released first and nothing tried twice on the device; the outputs are the same bytes.
// The store route (bam_store.h) sits between the two: when the whole stream is refused as over the cap and the store's
// planned need fits it, the file goes through the inflate's two slots as in the two-pass route, and behind the row
// kernels of every window the store's kernels copy each record's head, name and packed bases into one device allocation;
// pass B's kernels read that as they read the resident stream.  The file is inflated once and nothing of the inflated
// stream outlives its slot.  G2S_FILTER_STORE=1 takes the route even when the whole stream would fit, =0 never takes it.
// A planned capacity that proves too small (kTextStoreOverflow) releases the store and the rows, runs pass A again the
// two-pass way and pass B on the host: three passes, the same bytes.
// g2s_filter_reads_gaps_dpool (device_pool.h) is the pool form asking for one-pass mode by itself and keeping the text
// pass B's kernels wrote — the pooled build's layout, every read followed by 'N' — in device memory for the build to
// read there (g2s_graph_build_dpool_reach); only offsets and index lists come down.  Any other route gives the same
// handle with its text in host memory.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/g2s.h"
#include "../../include/g2s_test.h"
#include "bam.hpp"
#include "bam_rows.h"
#include "bam_text.h"
#include "device_pool.h"
#include "name_hash.h"
#include "readfilter_gaps.hpp"

namespace g2s {

namespace {

// fn(t, lo, hi) on `threads` threads over [0, n) cut into contiguous ranges, in range order by t
void parallel_ranges(size_t n, int threads, const std::function<void(int, size_t, size_t)>& fn) {
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), n / 4096 + 1));
  if (T == 1) { fn(0, 0, n); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(fn, t, n * (size_t)t / (size_t)T, n * (size_t)(t + 1) / (size_t)T);
  fn(0, 0, n / (size_t)T);
  for (auto& x : th) x.join();
}

// fn(i) for i in [0, n) on `threads` threads, dynamically (gaps differ a lot in work)
void parallel_items(size_t n, int threads, const std::function<void(size_t)>& fn) {
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), n));
  std::atomic<size_t> next{0};
  auto work = [&] { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i); };
  if (T == 1) { work(); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// The joins on host threads: the same steps as the device path (readfilter_gpu.hip), with sorted vectors and binary
// searches in place of its kernels.
int filter_join_host(FilterJoin& j, int threads, std::string* err) {
  const FilterRows& R = *j.rows;
  const size_t nr = R.size(), n = j.gaps();
  j.list1.clear();
  j.list2.clear();
  if (!nr || !j.bits || !n) return G2S_OK;  // (no records: the filter is empty and no window holds anything)
  // 1. the bits of every row's name and mate's name
  std::vector<uint64_t> b_own(nr), b_mate(nr);
  parallel_ranges(nr, threads, [&](int, size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) { b_own[r] = R.h_own[r] % j.bits; b_mate[r] = R.h_mate[r] % j.bits; }
  });
  // 2. the rows indexed by (ref_id, pos) — a coordinate-sorted file is its own index
  std::vector<uint64_t> ikey(nr);
  std::vector<uint32_t> irow(nr);
  for (size_t r = 0; r < nr; r++) { ikey[r] = filter_index_key(R.ref_id[r], R.pos[r]); irow[r] = (uint32_t)r; }
  if (!std::is_sorted(ikey.begin(), ikey.end())) {
    std::vector<std::pair<uint64_t, uint32_t>> kv(nr);
    for (size_t r = 0; r < nr; r++) kv[r] = {ikey[r], (uint32_t)r};
    std::sort(kv.begin(), kv.end());
    for (size_t r = 0; r < nr; r++) { ikey[r] = kv[r].first; irow[r] = kv[r].second; }
  }
  // the rows of a window: keys in [(tid, beg - max_span + 1), (tid, end)), then the overlap test on the end position
  auto window_rows = [&](const FilterWindow& w, const std::function<void(uint32_t)>& fn) {
    if (w.tid < 0 || w.beg >= w.end) return;
    const size_t lo = (size_t)(std::lower_bound(ikey.begin(), ikey.end(), filter_index_key(w.tid, w.beg - R.max_span + 1)) - ikey.begin());
    const size_t hi = (size_t)(std::lower_bound(ikey.begin(), ikey.end(), filter_index_key(w.tid, w.end)) - ikey.begin());
    for (size_t i = lo; i < hi; i++)
      if (R.end[irow[i]] > w.beg) fn(irow[i]);
  };
  // 3. every gap's filter: (bit << 29 | gap) of the mate-unmapped rows in its left and right windows, sorted, unique
  std::vector<std::vector<uint64_t>> per_gap(n);
  parallel_items(n, threads, [&](size_t g) {
    for (int w = 0; w < 2; w++)
      window_rows(j.win[3 * g + w], [&](uint32_t r) {
        if (R.flag[r] & BAM_MATE_UNMAPPED) per_gap[g].push_back(b_own[r] << kFilterGapBits | g);
      });
  });
  uint64_t pairs = 0;
  for (auto& v : per_gap) pairs += v.size();
  if (pairs > j.max_pairs) { *err = "more filter pairs than the cap (G2S_FILTER_MAX_PAIRS)"; return G2S_ERR_NOMEM; }
  std::vector<uint64_t> U;
  U.reserve((size_t)pairs);
  for (auto& v : per_gap) { U.insert(U.end(), v.begin(), v.end()); std::vector<uint64_t>().swap(v); }
  std::sort(U.begin(), U.end());
  U.erase(std::unique(U.begin(), U.end()), U.end());
  // 4. list 1: every row whose mate's bit is some gap's — one pair per such gap; rows in order within a gap (a
  // stable counting sort of the row ranges' pairs by gap)
  const int T = std::max(1, threads);
  std::vector<std::vector<uint64_t>> part((size_t)T);
  parallel_ranges(nr, threads, [&](int t, size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      const uint64_t m = b_mate[r];
      auto a = std::lower_bound(U.begin(), U.end(), m << kFilterGapBits);
      for (; a != U.end() && (*a >> kFilterGapBits) == m; ++a) part[(size_t)t].push_back((*a & kFilterGapMask) << 32 | r);
    }
  });
  uint64_t n1 = 0;
  for (auto& v : part) n1 += v.size();
  if (pairs + n1 > j.max_pairs) { *err = "more filter pairs than the cap (G2S_FILTER_MAX_PAIRS)"; return G2S_ERR_NOMEM; }
  {
    std::vector<uint64_t> at(n + 1, 0);
    for (auto& v : part)
      for (uint64_t x : v) at[(size_t)(x >> 32) + 1]++;
    for (size_t g = 0; g < n; g++) at[g + 1] += at[g];
    j.list1.resize((size_t)n1);
    for (auto& v : part) {
      for (uint64_t x : v) j.list1[(size_t)at[(size_t)(x >> 32)]++] = x;
      std::vector<uint64_t>().swap(v);
    }
  }
  // 5. list 2: per gap, the rows overlapping `around` whose own bit is not in the gap's filter, in row order
  std::vector<std::vector<uint32_t>> l2(n);
  parallel_items(n, threads, [&](size_t g) {
    window_rows(j.win[3 * g + 2], [&](uint32_t r) {
      if (!std::binary_search(U.begin(), U.end(), b_own[r] << kFilterGapBits | g)) l2[g].push_back(r);
    });
    std::sort(l2[g].begin(), l2[g].end());
  });
  uint64_t n2 = 0;
  for (auto& v : l2) n2 += v.size();
  if (pairs + n1 + n2 > j.max_pairs) { *err = "more filter pairs than the cap (G2S_FILTER_MAX_PAIRS)"; return G2S_ERR_NOMEM; }
  j.list2.reserve((size_t)n2);
  for (size_t g = 0; g < n; g++) {
    for (uint32_t r : l2[g]) j.list2.push_back((uint64_t)g << 32 | r);
    std::vector<uint32_t>().swap(l2[g]);
  }
  return G2S_OK;
}

namespace {

char* dup_text(const char* p, size_t n) {
  char* q = (char*)malloc(n + 1);
  if (!q) return nullptr;
  if (n) memcpy(q, p, n);
  q[n] = 0;
  return q;
}

// a malloc'ed copy of a vector's elements (one element at least, so that an empty array is not NULL)
template <class T>
T* dup_array(const T* p, size_t n) {
  T* q = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
  if (q && n) memcpy(q, p, n * sizeof(T));
  return q;
}

// Whether the reader inflates on the device when nothing says otherwise (G2S_HOST_INFLATE=1 / G2S_DEVICE_INFLATE=1).
// DESIGN 3.6b has the measurement this follows.
constexpr bool kDeviceInflateDefault = true;

bool env_is_1(const char* name) {
  const char* e = getenv(name);
  return e && strcmp(e, "1") == 0;
}

// g2s_test_last_filter_inflate: what the reader did in the process's last batched call
struct LastInflate {
  int on_device = 0;
  uint64_t members = 0, bytes_in = 0, bytes_out = 0;
  double ms_a = 0, ms_b = 0;
};
std::mutex g_last_mu;
LastInflate g_last;

// Whether pass A's rows are made on the device when the reader inflates there and nothing says otherwise
// (G2S_HOST_ROWS=1 / G2S_DEVICE_ROWS=1).  By DESIGN 3.6b's table the whole call with device rows is 32-35 ms faster than
// the parent's on average, more than the parent's own spread over six calls, with 8 and with 2 host threads.
constexpr bool kDeviceRowsDefault = true;

// g2s_test_last_filter_rows: what pass A of the process's last batched call (or g2s_test_bam_rows) did
struct LastRows {
  int on_device = 0, anomaly = 0;
  uint64_t windows = 0, records = 0, candidates = 0;
};
LastRows g_last_rows;

// g2s_filter_set_one_pass: -1 follows G2S_FILTER_ONE_PASS (read per call), 0 forbids, 1 asks
std::atomic<int> g_one_pass{-1};
bool one_pass_asked() {
  const int m = g_one_pass.load();
  return m < 0 ? env_is_1("G2S_FILTER_ONE_PASS") : m > 0;
}
// g2s_filter_reads_gaps_dpool asks by itself: a device-held pool is what the call is for.  Forbidding still forbids.
bool one_pass_asked_dpool() {
  const int m = g_one_pass.load();
  const char* e = getenv("G2S_FILTER_ONE_PASS");
  return m < 0 ? !(e && strcmp(e, "0") == 0) : m > 0;
}

// g2s_test_last_dpool: the process's last g2s_filter_reads_gaps_dpool[_mem]
LastDpoolFilter g_last_dpool;

// g2s_test_last_filter_text: what pass B of the process's last batched call did
struct LastText {
  int one_pass = 0, reason = kTextNotAsked;
  uint64_t reads = 0, bytes = 0, resident_bytes = 0;
};
LastText g_last_text;

// g2s_test_last_filter_store: the store route in pass A of the process's last batched call
StoreReport g_last_store;
// the store route's switches, read per call: G2S_FILTER_STORE (1 always, 0 never), G2S_FILTER_STORE_SAMPLE (bytes)
BamFile::StoreAsk store_ask_from_env() {
  BamFile::StoreAsk a;
  const char* e = getenv("G2S_FILTER_STORE");
  a.mode = e && strcmp(e, "1") == 0 ? 1 : e && strcmp(e, "0") == 0 ? 0 : -1;
  const char* b = getenv("G2S_FILTER_STORE_SAMPLE");
  const long long n = b ? atoll(b) : 0;
  a.sample = n > 0 ? (uint64_t)n : 0;
  return a;
}

// G2S_DEBUG=1: where a batched call's time outside its three laps goes — opening the file (the BGZF index and the header,
// whose first window zlib inflates), releasing run_filter_gaps' buffers, releasing the reader (its page-locked and device
// buffers).  Declared in front of the BamFile, so that it is destroyed behind it.
thread_local std::chrono::steady_clock::time_point g_laps_end;
struct OutsideLaps {
  using clock = std::chrono::steady_clock;
  clock::time_point enter = clock::now(), opened = enter, returned = enter;
  void open_done() { opened = clock::now(); }
  int run_done(int rc) { returned = clock::now(); return rc; }
  ~OutsideLaps() {
    if (returned == enter || !getenv("G2S_DEBUG")) return;
    auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[g2s] outside the laps: open %.1f ms, the call's buffers released in %.1f ms, the reader in %.1f ms\n",
            ms(enter, opened), ms(g_laps_end, returned), ms(returned, clock::now()));
  }
};

// pass A on the host: the walk, one row per record
bool pass_a_host(const BamFile& bam, FilterRows& R, int32_t* read_length, bool* too_many, std::string* err) {
  std::string nm;
  return bam.for_each([&](const BamRec& r) {
    if (R.size() >= (size_t)UINT32_MAX - 1) { *too_many = true; return false; }
    const int64_t e = r.end_pos();
    R.ref_id.push_back(r.ref_id);
    R.pos.push_back(r.pos);
    R.end.push_back(e);
    R.flag.push_back(r.flag);
    nm.assign(r.name, strnlen(r.name, r.l_name));
    const bool r1 = (r.flag & BAM_READ1) != 0;
    nm += r1 ? "/1" : "/2";
    R.h_own.push_back((uint64_t)std::hash<std::string>{}(nm));
    nm.back() = r1 ? '2' : '1';
    R.h_mate.push_back((uint64_t)std::hash<std::string>{}(nm));
    *read_length = std::max(*read_length, r.l_seq);
    if (r.ref_id >= 0) R.max_span = std::max(R.max_span, e - (int64_t)r.pos);
    return true;
  }, err);
}

// The probe of name_hash.h against this build's std::hash<std::string>: names of every length 0 to 40 and of 254,
// bytes >= 0x80 in each of a name's last seven positions, names with a NUL inside (the part in front counts) and 500
// names of random bytes, each with /1 and /2.  tests/bam_walk_cases.py's hash_names() builds the same names from the
// same generator (xorshift64 from 0x9E3779B97F4A7C15, one draw a byte), so the tests pin what a process checks.
bool name_hash_probe() {
  std::vector<std::string> names;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  auto printable = [&](size_t len) {
    std::string s;
    for (size_t i = 0; i < len; i++) s.push_back((char)('!' + next() % 94));
    return s;
  };
  for (size_t len = 0; len <= 40; len++) names.push_back(printable(len));
  names.push_back(printable(254));
  for (size_t len : {7u, 8u, 9u, 15u, 16u, 23u})
    for (size_t back = 1; back <= 7; back++) {
      std::string s(len, 'a');
      s[len - back] = (char)(0x80 + next() % 128);
      names.push_back(s);
    }
  for (const std::string& s : {std::string("ab\0cd", 5), std::string("\0zzz", 4), std::string("abcdefg\0hij\0", 12),
                               std::string("abcdefgh\0", 9)})
    names.push_back(s.substr(0, strnlen(s.data(), s.size())));
  for (int i = 0; i < 500; i++) {
    std::string s;
    const size_t len = next() % 64;
    for (size_t k = 0; k < len; k++) s.push_back((char)(1 + next() % 255));
    names.push_back(s);
  }
  for (const std::string& s : names)
    for (uint32_t which = 1; which <= 2; which++) {
      const std::string full = s + (which == 1 ? "/1" : "/2");
      if ((uint64_t)std::hash<std::string>{}(full) != name_hash((const uint8_t*)s.data(), (uint32_t)s.size(), which)) return false;
    }
  return true;
}
bool name_hash_usable() {
  static const bool ok = name_hash_probe();  // once a process
  return ok;
}

// Pass A on the device.  Null: *anomaly says why (kRowsOk: nothing asked for it), the reader's statistics are as they
// were, and the host walk runs.
std::unique_ptr<BamRowsDevice> pass_a_device(const BamFile& bam, size_t walk_window, int* anomaly, bool resident = false,
                                             int* resident_refused = nullptr, const BamFile::StoreAsk* store = nullptr) {
  std::string why;
  *anomaly = kRowsOk;
  std::unique_ptr<BamRowsDevice> D;
  if (!name_hash_usable()) {
    *anomaly = kRowsHash;
    why = "name_hash.h is not this build's std::hash<std::string>";
  } else {
    const char* cap = getenv("G2S_FILTER_RESIDENT_CAP");
    D.reset(bam.rows_on_device(walk_window, anomaly, &why, resident, cap ? (uint64_t)strtoull(cap, nullptr, 10) : 0,
                               resident_refused, nullptr, store));
  }
  if (!D && getenv("G2S_DEBUG"))
    fprintf(stderr, "[g2s] pass A: no device rows (anomaly %d: %s): the host walk\n", *anomaly, why.c_str());
  if (D && getenv("G2S_DEBUG")) fprintf(stderr, "[g2s] pass A: rows on the device (%zu windows)\n", (size_t)bam.rows_windows());
  return D;
}

// pass B on the host: a second walk over the file, for the rows of `sel` (and the unmapped reads when asked for)
bool pass_b_host(const BamFile& bam, uint64_t total, const std::vector<uint8_t>& sel, const BamTextAsk& ask, BamText* T,
                 uint64_t* rows_seen, std::string* err) {
  *T = BamText();
  if (ask.pool) T->pidx.assign((size_t)total, 0);
  else { T->toff.assign((size_t)total, 0); T->tlen.assign((size_t)total, 0); }
  size_t row = 0;
  const bool ok = bam.for_each([&](const BamRec& r) {
    if (row >= total) return false;  // (the file changed under us: the caller's guard)
    if (ask.pool) {
      const bool un = ask.unmapped && (r.flag & BAM_UNMAPPED);
      if (sel[row] || un) {
        T->pidx[row] = (uint32_t)(T->pboff.size() - 1);
        if (un) T->punmapped.push_back(T->pidx[row]);
        append_bases(r, &T->pbases);
        T->pboff.push_back(T->pbases.size());
        if (ask.names) { T->pnames += own_name(r); T->pnoff.push_back(T->pnames.size()); }
      }
      row++;
      return true;
    }
    if (sel[row]) {
      T->toff[row] = T->text.size();
      append_fasta(r, &T->text);
      T->tlen[row] = (uint32_t)(T->text.size() - T->toff[row]);
    }
    if (ask.unmapped && (r.flag & BAM_UNMAPPED)) { append_fasta(r, &T->unmapped); T->n_unmapped++; }
    row++;
    return true;
  }, err);
  *rows_seen = row;
  return ok;
}

// what g2s_filter_reads_gaps_pool asks of run_filter_gaps in place of the per-gap texts
// (dout: g2s_filter_reads_gaps_dpool — the pool as a g2s_device_pool, its bases left on the device when pass B ran there)
struct PoolRequest {
  bool names, unmapped;
  g2s_read_pool** out;
  g2s_device_pool** dout = nullptr;
};

int run_filter_gaps(BamFile& bam, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n, int device,
                    char** fasta_out, char** log_out, char** warn_out, int64_t* extracted_out, int64_t* total_out,
                    char** unmapped_out, int64_t* unmapped_extracted, g2s_filter_stats* stats,
                    const PoolRequest* pool = nullptr) {
  std::string err;
  g2s_filter_stats st;
  memset(&st, 0, sizeof st);
  const int threads = lib->threads > 0 ? lib->threads : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  bam.set_threads(threads);
  // the reader inflates where the joins run, by the same rule, unless a switch says otherwise
  const bool device_wanted = device >= 0 && !env_is_1("G2S_HOST_FILTER");
  const bool device_inflate = device_wanted && !env_is_1("G2S_HOST_INFLATE") &&
                              (kDeviceInflateDefault || env_is_1("G2S_DEVICE_INFLATE")) && filter_device_usable(device);
  bam.set_inflate_device(device_inflate ? device : -1);
  bam.reset_inflate_stats();
  LastInflate li;
  bool all_device = device_inflate;
  auto note_pass = [&](double* ms) {
    const BamFile::InflateStats& is = bam.inflate_stats();
    *ms = is.ms_refill;
    li.members += is.members;
    li.bytes_in += is.bytes_in;
    li.bytes_out += is.bytes_out;
    if (is.host_windows || !is.device_windows) all_device = false;
    li.on_device = all_device ? 1 : 0;
    bam.reset_inflate_stats();
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last = li;
  };
  // ---- pass A
  auto t0 = std::chrono::steady_clock::now();
  FilterRows R;
  int32_t read_length = 0;
  bool too_many = false;
  st.file_passes++;
  // the rows on the device, under the rule that inflates there, unless a switch says otherwise
  std::unique_ptr<BamRowsDevice> drows;
  LastRows lr;
  // one-pass mode: asked for, and then whatever stands in its way is the reason it did not run
  LastText lt;
  StoreReport ls;
  bool store_overflow = false;
  const bool dpool = pool && pool->dout;
  const bool asked = dpool ? one_pass_asked_dpool() : one_pass_asked();
  lt.reason = asked ? kTextNoDeviceRows : kTextNotAsked;
  if (device_inflate && !env_is_1("G2S_HOST_ROWS") && (kDeviceRowsDefault || env_is_1("G2S_DEVICE_ROWS"))) {
    int refused = kResidentKept;
    const BamFile::StoreAsk sa = store_ask_from_env();
    drows = pass_a_device(bam, 0, &lr.anomaly, asked, &refused, asked ? &sa : nullptr);
    lr.windows = bam.rows_windows();
    if (asked) ls = bam.store_report();
    if (!drows) bam.reset_inflate_stats();
    if (!drows && ls.overflow) {
      // a planned capacity was too small: the store and the rows are gone, and pass A runs again the two-pass way
      if (getenv("G2S_DEBUG"))
        fprintf(stderr, "[g2s] store route given up: the planned %s overflowed (rows %llu, store %llu bytes): pass A again\n",
                ls.overflow == 1 ? "rows" : "store", (unsigned long long)ls.rows_cap, (unsigned long long)ls.store_cap);
      st.file_passes++;
      store_overflow = true;
      drows = pass_a_device(bam, 0, &lr.anomaly, false, nullptr);
      lr.windows = bam.rows_windows();
      if (!drows) bam.reset_inflate_stats();
    }
    if (store_overflow) lt.reason = kTextStoreOverflow;
    else if (asked && refused != kResidentKept) lt.reason = refused == kResidentOverCap ? kTextOverCap : kTextFailed;
    else if (asked && drows && drows->stream_buffer()) lt.resident_bytes = drows->stream_bytes();
  }
  const bool resident = drows && drows->stream_buffer();
  if (asked && getenv("G2S_DEBUG")) {
    static const char* const kWhy[] = {"", "", "pass A's rows were not made on the device", "over the cap", "an allocation failed",
                                       "a planned capacity of the store route overflowed"};
    if (resident && ls.used)
      fprintf(stderr, "[g2s] one-pass route: the records' heads, names and bases stay on the device (store %llu of %llu bytes, "
                      "rows %llu of %llu, need %llu bytes)\n", (unsigned long long)ls.store_bytes, (unsigned long long)ls.store_cap,
              (unsigned long long)ls.records, (unsigned long long)ls.rows_cap, (unsigned long long)ls.device_bytes);
    else if (resident) fprintf(stderr, "[g2s] one-pass route: the inflated file stays on the device (%llu bytes)\n",
                               (unsigned long long)lt.resident_bytes);
    else fprintf(stderr, "[g2s] two-pass route (%s)\n", kWhy[lt.reason]);
  }
  auto note_text = [&] {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last_text = lt;
    g_last_store = ls;
  };
  note_text();
  if (drows) {
    lr.on_device = 1;
    lr.records = drows->rows().n;
    lr.candidates = drows->candidates();
    read_length = drows->rows().read_length;
    R.max_span = drows->rows().max_span;
  }
  {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last_rows = lr;
  }
  if (!drows && !pass_a_host(bam, R, &read_length, &too_many, &err)) {
    note_pass(&li.ms_a);
    set_filter_error(err);
    return G2S_ERR_IO;
  }
  note_pass(&li.ms_a);
  if (too_many) { set_filter_error("more than 2^32 - 2 records"); return G2S_ERR_ARG; }
  st.ms_inflate = ms_since(t0);
  const uint64_t total = drows ? drows->rows().n : R.size();
  if (!drows) {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last_rows.records = total;
  }
  // ---- every gap's windows and warnings (readfilter.cpp: run_filter)
  t0 = std::chrono::steady_clock::now();
  FilterJoin J;
  J.rows = &R;
  if (drows) J.device_rows = &drows->rows();
  J.bits = 5 * total;
  const char* cap = getenv("G2S_FILTER_MAX_PAIRS");
  J.max_pairs = cap ? (uint64_t)strtoull(cap, nullptr, 10) : (uint64_t)1 << 31;
  J.win.resize(3 * n);
  std::vector<std::string> warn(n);
  for (size_t i = 0; i < n; i++) {
    const g2s_filter_gap& g = gaps[i];
    const int tid = bam.ref_id(g.scaffold ? g.scaffold : "");
    const int64_t bp = g.breakpoint, mu = lib->mean_insert, sd = lib->std_dev, gl = g.gap_length, rl = read_length;
    J.win[3 * i] = filter_window(make_region(tid, bp - (mu + 3 * sd + 2 * rl), bp - (mu - 3 * sd + rl), &warn[i]));
    J.win[3 * i + 1] = filter_window(make_region(tid, bp + (mu + 3 * sd + rl) + gl, bp + (mu - 3 * sd + rl) + gl, &warn[i]));
    if (g.flank_length != -1)
      J.win[3 * i + 2] = filter_window(make_region(tid, bp - (int64_t)g.flank_length, bp + (int64_t)g.flank_length + gl, &warn[i]));
    else
      J.win[3 * i + 2] = FilterWindow{-1, 0, 0, 0};
  }
  // ---- the joins
  const bool on_device = device_wanted && filter_device_usable(device);
  const int rc = on_device ? filter_join_device(J, device, &err) : filter_join_host(J, threads, &err);
  if (rc != G2S_OK) { set_filter_error(err); return rc; }
  st.on_device = on_device ? 1 : 0;
  st.ms_join = ms_since(t0);
  if (!resident) drows.reset();
  // ---- pass B: the text of the selected rows
  t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> sel(total, 0);
  for (uint64_t x : J.list1) sel[(uint32_t)x] = 1;
  for (uint64_t x : J.list2) sel[(uint32_t)x] = 1;
  BamTextAsk ask;
  ask.pool = pool != nullptr;
  ask.names = pool && pool->names;
  ask.unmapped = pool ? pool->unmapped : unmapped_out != nullptr;
  ask.device_text = dpool;
  BamText T;
  // (a text left on the device belongs to the handle made below; until then it goes with this scope)
  struct TextGuard {
    BamText& t;
    ~TextGuard() { if (t.d_text) device_pool_release(t.d_device, t.d_text); }
  } text_guard{T};
  bool text_done = false;
  if (resident) {  // (one-pass mode: from the stream pass A left on the device)
    std::string why;
    const double ms_sel = ms_since(t0);
    text_done = bam_text_device(*drows, sel.data(), ask, &T, &why);
    const double ms_dev = ms_since(t0);
    drows.reset();  // (the resident buffer goes before anything else runs)
    if (getenv("G2S_DEBUG"))
      fprintf(stderr, "[g2s] pass B on the device: selection %.1f ms, kernels and copies %.1f ms, release %.1f ms\n", ms_sel,
              ms_dev - ms_sel, ms_since(t0) - ms_dev);
    if (text_done) {
      lt.one_pass = 1;
      lt.reason = kTextOnDevice;
      lt.reads = pool ? T.pboff.size() - 1 : (uint64_t)std::count(sel.begin(), sel.end(), (uint8_t)1) + (uint64_t)T.n_unmapped;
      lt.bytes = pool ? T.pbases.size() + T.pnames.size() : T.text.size() + T.unmapped.size();
    } else {
      lt.reason = kTextFailed;
      ls.used = 0;
      if (getenv("G2S_DEBUG")) fprintf(stderr, "[g2s] one-pass route given up in pass B (%s): the second pass on the host\n", why.c_str());
    }
    note_text();
  }
  if (!text_done) {
    uint64_t row = 0;
    st.file_passes++;
    const bool ok = pass_b_host(bam, total, sel, ask, &T, &row, &err);
    note_pass(&li.ms_b);
    if (!ok) { set_filter_error(err); return G2S_ERR_IO; }
    if (row != total) { set_filter_error("the BAM file changed between passes"); return G2S_ERR_IO; }
  }
  const std::vector<uint64_t>&toff = T.toff, &pboff = T.pboff, &pnoff = T.pnoff;
  const std::vector<uint32_t>&tlen = T.tlen, &pidx = T.pidx, &punmapped = T.punmapped;
  const std::string &text = T.text, &unmapped = T.unmapped, &pbases = T.pbases, &pnames = T.pnames;
  const int64_t n_unmapped = T.n_unmapped;
  const bool want_unmapped = ask.unmapped;
  // ---- every gap's text: list 1's rows, then list 2's
  std::vector<size_t> at1(n + 1, 0), at2(n + 1, 0);
  for (uint64_t x : J.list1) at1[(size_t)(x >> 32) + 1]++;
  for (uint64_t x : J.list2) at2[(size_t)(x >> 32) + 1]++;
  for (size_t g = 0; g < n; g++) { at1[g + 1] += at1[g]; at2[g + 1] += at2[g]; }
  if (pool) {  // ... as indices into the pool, in the same order
    std::vector<uint64_t> gbeg(n + 1, 0);
    std::vector<uint32_t> gread(J.list1.size() + J.list2.size());
    for (size_t g = 0; g < n; g++) {
      size_t o = (size_t)gbeg[g];
      for (size_t q = at1[g]; q < at1[g + 1]; q++) gread[o++] = pidx[(uint32_t)J.list1[q]];
      for (size_t q = at2[g]; q < at2[g + 1]; q++) gread[o++] = pidx[(uint32_t)J.list2[q]];
      gbeg[g + 1] = o;
    }
    if (dpool) {  // ... as a handle that owns the same arrays, and the text where pass B left it
      g2s_device_pool* H = new (std::nothrow) g2s_device_pool();
      if (!H) { set_filter_error("out of memory"); return G2S_ERR_NOMEM; }
      LastDpoolFilter ld;
      try {
        H->base_off = pboff;
        H->name_off = pnoff;
        H->gap_begin.swap(gbeg);
        H->gap_read.swap(gread);
        H->unmapped_read = punmapped;
        if (T.d_text) {
          H->device = T.d_device;
          H->d_text = T.d_text;
          H->d_start = T.d_start;
          H->device_bytes = T.d_bytes;
          T.d_text = nullptr;
          ld.held_on_device = 1;
        } else {  // (host-held: the build's layout, so that both kinds read alike)
          H->host_text.resize((size_t)H->text_bytes());
          for (size_t r = 0; r + 1 < pboff.size(); r++) {
            const size_t len = (size_t)(pboff[r + 1] - pboff[r]), at = (size_t)H->start(r);
            if (len) memcpy(&H->host_text[at], pbases.data() + pboff[r], len);
            H->host_text[at + len] = 'N';
          }
          ld.bases_bytes_to_host = pbases.size();
        }
        H->gap_read.reserve(1);  // (one element at least behind every pointer, as g2s_read_pool's arrays have)
        H->unmapped_read.reserve(1);
      } catch (const std::bad_alloc&) {
        g2s_device_pool_free(H);
        set_filter_error("out of memory");
        return G2S_ERR_NOMEM;
      }
      H->view.n_reads = H->base_off.size() - 1;
      H->view.base_off = H->base_off.data();
      H->view.name_off = H->name_off.data();
      H->view.gap_begin = H->gap_begin.data();
      H->view.gap_read = H->gap_read.data();
      H->view.n_unmapped = H->unmapped_read.size();
      H->view.unmapped_read = H->unmapped_read.data();
      *pool->dout = H;
      {
        std::lock_guard<std::mutex> lk(g_last_mu);
        g_last_dpool = ld;
      }
      if (total_out) *total_out = (int64_t)total;
      st.ms_text = ms_since(t0);
      if (stats) *stats = st;
      g_laps_end = std::chrono::steady_clock::now();
      return G2S_OK;
    }
    g2s_read_pool* P =(g2s_read_pool*)calloc(1, sizeof(g2s_read_pool));
    if (P) {
      P->n_reads = pboff.size() - 1;
      P->bases = dup_array(pbases.data(), pbases.size());
      P->base_off = dup_array(pboff.data(), pboff.size());
      if (pool->names) {
        P->names = dup_array(pnames.data(), pnames.size());
        P->name_off = dup_array(pnoff.data(), pnoff.size());
      }
      P->gap_begin = dup_array(gbeg.data(), gbeg.size());
      P->gap_read = dup_array(gread.data(), gread.size());
      P->n_unmapped = punmapped.size();
      P->unmapped_read = dup_array(punmapped.data(), punmapped.size());
    }
    if (!P || !P->bases || !P->base_off || (pool->names && (!P->names || !P->name_off)) || !P->gap_begin || !P->gap_read ||
        !P->unmapped_read) {
      g2s_read_pool_free(P);
      set_filter_error("out of memory");
      return G2S_ERR_NOMEM;
    }
    *pool->out = P;
    if (total_out) *total_out = (int64_t)total;
    st.ms_text = ms_since(t0);
    if (stats) *stats = st;
    g_laps_end = std::chrono::steady_clock::now();
    return G2S_OK;
  }
  std::vector<char*> fa(n, nullptr), lg(n, nullptr), wn(n, nullptr);
  std::atomic<bool> oom{false};
  parallel_items(n, threads, [&](size_t g) {
    size_t bytes = 0;
    for (size_t q = at1[g]; q < at1[g + 1]; q++) bytes += tlen[(uint32_t)J.list1[q]];
    for (size_t q = at2[g]; q < at2[g + 1]; q++) bytes += tlen[(uint32_t)J.list2[q]];
    if (fasta_out) {
      char* p = (char*)malloc(bytes + 1);
      if (!p) { oom = true; return; }
      size_t o = 0;
      for (size_t q = at1[g]; q < at1[g + 1]; q++) { const uint32_t r = (uint32_t)J.list1[q]; memcpy(p + o, text.data() + toff[r], tlen[r]); o += tlen[r]; }
      for (size_t q = at2[g]; q < at2[g + 1]; q++) { const uint32_t r = (uint32_t)J.list2[q]; memcpy(p + o, text.data() + toff[r], tlen[r]); o += tlen[r]; }
      p[o] = 0;
      fa[g] = p;
    }
    const int64_t ex = (int64_t)(at1[g + 1] - at1[g] + at2[g + 1] - at2[g]);
    if (extracted_out) extracted_out[g] = ex;
    if (log_out) {
      const std::string log = "Extracted " + std::to_string(ex) + " out of " + std::to_string(total) + " reads\n";  // :406
      if (!(lg[g] = dup_text(log.data(), log.size()))) oom = true;
    }
    if (warn_out && !(wn[g] = dup_text(warn[g].data(), warn[g].size()))) oom = true;
  });
  char* un = nullptr;
  if (want_unmapped && !(un = dup_text(unmapped.data(), unmapped.size()))) oom = true;
  if (oom) {
    for (size_t g = 0; g < n; g++) { free(fa[g]); free(lg[g]); free(wn[g]); }
    free(un);
    set_filter_error("out of memory");
    return G2S_ERR_NOMEM;
  }
  for (size_t g = 0; g < n; g++) {
    if (fasta_out) fasta_out[g] = fa[g];
    if (log_out) log_out[g] = lg[g];
    if (warn_out) warn_out[g] = wn[g];
  }
  if (want_unmapped) *unmapped_out = un;
  if (unmapped_extracted) *unmapped_extracted = n_unmapped;
  if (total_out) *total_out = (int64_t)total;
  st.ms_text = ms_since(t0);
  if (stats) *stats = st;
  g_laps_end = std::chrono::steady_clock::now();
  return G2S_OK;
}

bool gap_args_ok(const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n) {
  if (!lib || (n && !gaps)) { set_filter_error("null argument"); return false; }
  if (n > kFilterGapMask) { set_filter_error("more than 2^29 - 1 gaps in one call"); return false; }
  return true;
}

}  // namespace

LastDpoolFilter last_dpool_filter() {
  std::lock_guard<std::mutex> lk(g_last_mu);
  return g_last_dpool;
}

}  // namespace g2s

extern "C" {

int g2s_filter_reads_gaps(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n, int device,
                          char** fasta_out, char** log_out, char** warn_out, int64_t* extracted, int64_t* total,
                          char** unmapped_out, int64_t* unmapped_extracted, g2s_filter_stats* stats) {
  if (!bam_path || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_path(bam_path, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, fasta_out, log_out, warn_out, extracted, total,
                                            unmapped_out, unmapped_extracted, stats));
}

int g2s_filter_reads_gaps_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                              size_t n, int device, char** fasta_out, char** log_out, char** warn_out, int64_t* extracted,
                              int64_t* total, char** unmapped_out, int64_t* unmapped_extracted, g2s_filter_stats* stats) {
  if (!bam_bytes || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bam_bytes, nbytes, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, fasta_out, log_out, warn_out, extracted, total,
                                            unmapped_out, unmapped_extracted, stats));
}

int g2s_filter_reads_gaps_pool(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n, int device,
                               int want_names, int want_unmapped, g2s_read_pool** out, int64_t* total, g2s_filter_stats* stats) {
  if (!bam_path || !out || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_path(bam_path, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  const g2s::PoolRequest req{want_names != 0, want_unmapped != 0, out};
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, nullptr, nullptr, nullptr, nullptr, total, nullptr, nullptr,
                                            stats, &req));
}

int g2s_filter_reads_gaps_pool_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                                   size_t n, int device, int want_names, int want_unmapped, g2s_read_pool** out, int64_t* total,
                                   g2s_filter_stats* stats) {
  if (!bam_bytes || !out || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bam_bytes, nbytes, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  const g2s::PoolRequest req{want_names != 0, want_unmapped != 0, out};
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, nullptr, nullptr, nullptr, nullptr, total, nullptr, nullptr,
                                            stats, &req));
}

int g2s_filter_reads_gaps_dpool(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n, int device,
                                int want_unmapped, g2s_device_pool** out, int64_t* total, g2s_filter_stats* stats) {
  if (!bam_path || !out || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_path(bam_path, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  const g2s::PoolRequest req{true, want_unmapped != 0, nullptr, out};
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, nullptr, nullptr, nullptr, nullptr, total, nullptr, nullptr,
                                            stats, &req));
}

int g2s_filter_reads_gaps_dpool_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                                    size_t n, int device, int want_unmapped, g2s_device_pool** out, int64_t* total,
                                    g2s_filter_stats* stats) {
  if (!bam_bytes || !out || !g2s::gap_args_ok(lib, gaps, n)) return G2S_ERR_ARG;
  g2s::OutsideLaps laps;
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bam_bytes, nbytes, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  laps.open_done();
  const g2s::PoolRequest req{true, want_unmapped != 0, nullptr, out};
  return laps.run_done(g2s::run_filter_gaps(bam, lib, gaps, n, device, nullptr, nullptr, nullptr, nullptr, total, nullptr, nullptr,
                                            stats, &req));
}

const g2s_read_pool* g2s_device_pool_view(const g2s_device_pool* p) { return p ? &p->view : nullptr; }
int g2s_device_pool_device(const g2s_device_pool* p) { return p ? p->device : -1; }
uint64_t g2s_device_pool_bytes(const g2s_device_pool* p) { return p ? p->device_bytes : 0; }

int g2s_device_pool_read(const g2s_device_pool* p, uint64_t r, char* out) {
  if (!p || r >= p->view.n_reads) { g2s::set_filter_error("g2s_device_pool_read: bad argument"); return G2S_ERR_ARG; }
  const uint64_t len = p->base_off[(size_t)r + 1] - p->base_off[(size_t)r];
  if (!len) return G2S_OK;
  if (!out) { g2s::set_filter_error("g2s_device_pool_read: bad argument"); return G2S_ERR_ARG; }
  if (p->device < 0) { memcpy(out, p->host_text.data() + p->start(r), (size_t)len); return G2S_OK; }
  std::string why;
  if (!g2s::device_pool_copy_down(p->device, p->d_text, p->start(r), len, out, &why)) { g2s::set_filter_error(why); return G2S_ERR_HIP; }
  return G2S_OK;
}

void g2s_device_pool_free(g2s_device_pool* p) {
  if (!p) return;
  if (p->d_text) g2s::device_pool_release(p->device, p->d_text);  // (sets the handle's device first)
  delete p;
}

void g2s_read_pool_free(g2s_read_pool* p) {
  if (!p) return;
  free(p->bases);
  free(p->base_off);
  free(p->names);
  free(p->name_off);
  free(p->gap_begin);
  free(p->gap_read);
  free(p->unmapped_read);
  free(p);
}

// TEST HOOK (include/g2s_test.h): a whole BGZF file through one of the three inflaters.
int g2s_test_bgzf_inflate(const void* bytes, size_t n, int device, uint8_t* out, size_t cap, size_t* out_n, int64_t* bad_member) {
  if (!bytes || !out_n || (cap && !out) || device < -2) {
    g2s::set_filter_error("g2s_test_bgzf_inflate: bad argument");
    return G2S_ERR_ARG;
  }
  *out_n = 0;
  if (bad_member) *bad_member = -1;
  if (device >= 0 && !g2s::filter_device_usable(device)) {
    g2s::set_filter_error("g2s_test_bgzf_inflate: no usable gfx950 device " + std::to_string(device));
    return G2S_ERR_NO_DEVICE;
  }
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_bgzf(bytes, n, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  bam.set_threads(1);
  bam.set_inflate_core(device == -2);
  bam.set_inflate_device(device >= 0 ? device : -1);
  bam.reset_inflate_stats();
  std::vector<uint8_t> all;
  int64_t bad = -1;
  const bool ok = bam.read_all(&all, &err, &bad);
  if (device >= 0 && bam.inflate_stats().host_windows) {  // (never the host in the kernel's place)
    g2s::set_filter_error("g2s_test_bgzf_inflate: the device refused");
    return G2S_ERR_HIP;
  }
  if (!ok) {
    if (bad_member) *bad_member = bad;
    g2s::set_filter_error(err);
    return G2S_ERR_IO;
  }
  g2s::set_filter_error("");
  *out_n = all.size();
  if (cap && !all.empty()) memcpy(out, all.data(), std::min(cap, all.size()));
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h)
int g2s_test_last_filter_inflate(int* on_device, uint64_t* members, uint64_t* bytes_in, uint64_t* bytes_out,
                                 double* ms_pass_a_inflate, double* ms_pass_b_inflate) {
  std::lock_guard<std::mutex> lk(g2s::g_last_mu);
  if (on_device) *on_device = g2s::g_last.on_device;
  if (members) *members = g2s::g_last.members;
  if (bytes_in) *bytes_in = g2s::g_last.bytes_in;
  if (bytes_out) *bytes_out = g2s::g_last.bytes_out;
  if (ms_pass_a_inflate) *ms_pass_a_inflate = g2s::g_last.ms_a;
  if (ms_pass_b_inflate) *ms_pass_b_inflate = g2s::g_last.ms_b;
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h)
int g2s_test_last_filter_text(int* one_pass, int* reason, uint64_t* reads, uint64_t* bytes, uint64_t* resident_bytes) {
  std::lock_guard<std::mutex> lk(g2s::g_last_mu);
  if (one_pass) *one_pass = g2s::g_last_text.one_pass;
  if (reason) *reason = g2s::g_last_text.reason;
  if (reads) *reads = g2s::g_last_text.reads;
  if (bytes) *bytes = g2s::g_last_text.bytes;
  if (resident_bytes) *resident_bytes = g2s::g_last_text.resident_bytes;
  return G2S_OK;
}

int g2s_filter_set_one_pass(int mode) { return g2s::g_one_pass.exchange(mode < 0 ? -1 : mode > 0 ? 1 : 0); }

// pass B alone (g2s_test_bam_text; `store`: g2s_test_bam_text_store, pass A in store form at the walk window `window`)
static int bam_text_hook(bool store, size_t window, const void* bytes, size_t n, int device, const uint32_t* rows, uint64_t n_rows,
                         int want_names, int fasta, uint8_t* bases, uint64_t bases_cap, uint64_t* bases_n, uint8_t* names,
                         uint64_t names_cap, uint64_t* names_n, uint64_t* base_off, uint64_t* name_off, uint64_t off_cap,
                         uint64_t* n_reads) {
  if (!bytes || (n_rows && !rows) || !bases_n || !names_n || !n_reads || (bases_cap && !bases) || (names_cap && !names) ||
      (off_cap && (!base_off || !name_off))) {
    g2s::set_filter_error("g2s_test_bam_text: bad argument");
    return G2S_ERR_ARG;
  }
  *bases_n = *names_n = *n_reads = 0;
  if (device >= 0 && !g2s::filter_device_usable(device)) {
    g2s::set_filter_error("g2s_test_bam_text: no usable gfx950 device " + std::to_string(device));
    return G2S_ERR_NO_DEVICE;
  }
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bytes, n, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  bam.set_threads(1);
  bam.set_inflate_device(device >= 0 ? device : -1);
  // pass A, for the record count (and, on the device, the resident stream)
  std::unique_ptr<g2s::BamRowsDevice> D;
  uint64_t total = 0;
  if (device >= 0) {
    int anomaly = 0, refused = 0;
    g2s::BamFile::StoreAsk sa;  // (no switch is read: the store always, at the capacities that cannot overflow)
    sa.mode = 1;
    sa.worst_case = true;
    D = g2s::pass_a_device(bam, store ? window : 0, &anomaly, true, &refused, store ? &sa : nullptr);
    if (!D || !D->stream_buffer() || D->store_form() != store) {  // (never the host in the kernels' place)
      g2s::set_filter_error("g2s_test_bam_text: no resident stream (anomaly " + std::to_string(anomaly) + ", refused " +
                            std::to_string(refused) + ")");
      return G2S_ERR_HIP;
    }
    total = D->rows().n;
  } else {
    g2s::FilterRows R;
    int32_t rl = 0;
    bool too_many = false;
    if (!g2s::pass_a_host(bam, R, &rl, &too_many, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
    if (too_many) { g2s::set_filter_error("more than 2^32 - 2 records"); return G2S_ERR_ARG; }
    total = R.size();
  }
  std::vector<uint8_t> sel((size_t)total, 0);
  for (uint64_t i = 0; i < n_rows; i++) {
    if (rows[i] >= total) { g2s::set_filter_error("g2s_test_bam_text: a row beyond the file's records"); return G2S_ERR_ARG; }
    sel[rows[i]] = 1;
  }
  g2s::BamTextAsk ask;
  ask.pool = !fasta;
  ask.names = !fasta && want_names;
  g2s::BamText T;
  if (device >= 0) {
    if (!g2s::bam_text_device(*D, sel.data(), ask, &T, &err)) { g2s::set_filter_error("g2s_test_bam_text: " + err); return G2S_ERR_HIP; }
  } else {
    uint64_t seen = 0;
    if (!g2s::pass_b_host(bam, total, sel, ask, &T, &seen, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  }
  // the selected rows' pieces in file order: the pool's arrays, or the FASTA records with their offsets
  std::vector<uint64_t> foff(1, 0);
  std::string ftext;
  if (fasta)
    for (size_t r = 0; r < (size_t)total; r++)
      if (sel[r]) { ftext.append(T.text, (size_t)T.toff[r], T.tlen[r]); foff.push_back(ftext.size()); }
  const std::string& B = fasta ? ftext : T.pbases;
  const std::vector<uint64_t>& BO = fasta ? foff : T.pboff;
  *n_reads = BO.size() - 1;
  *bases_n = B.size();
  *names_n = T.pnames.size();
  if (bases_cap && !B.empty()) memcpy(bases, B.data(), (size_t)std::min<uint64_t>(bases_cap, B.size()));
  if (names_cap && !T.pnames.empty()) memcpy(names, T.pnames.data(), (size_t)std::min<uint64_t>(names_cap, T.pnames.size()));
  for (uint64_t i = 0; i < std::min<uint64_t>(off_cap, BO.size()); i++) {
    base_off[i] = BO[i];
    name_off[i] = ask.names ? T.pnoff[i] : 0;
  }
  g2s::set_filter_error("");
  return G2S_OK;
}

// TEST HOOKS (include/g2s_test.h)
int g2s_test_bam_text(const void* bytes, size_t n, int device, const uint32_t* rows, uint64_t n_rows, int want_names, int fasta,
                      uint8_t* bases, uint64_t bases_cap, uint64_t* bases_n, uint8_t* names, uint64_t names_cap,
                      uint64_t* names_n, uint64_t* base_off, uint64_t* name_off, uint64_t off_cap, uint64_t* n_reads) {
  return bam_text_hook(false, 0, bytes, n, device, rows, n_rows, want_names, fasta, bases, bases_cap, bases_n, names, names_cap,
                       names_n, base_off, name_off, off_cap, n_reads);
}
int g2s_test_bam_text_store(const void* bytes, size_t n, int device, size_t window, const uint32_t* rows, uint64_t n_rows,
                            int want_names, int fasta, uint8_t* bases, uint64_t bases_cap, uint64_t* bases_n, uint8_t* names,
                            uint64_t names_cap, uint64_t* names_n, uint64_t* base_off, uint64_t* name_off, uint64_t off_cap,
                            uint64_t* n_reads) {
  return bam_text_hook(device >= 0, window, bytes, n, device, rows, n_rows, want_names, fasta, bases, bases_cap, bases_n, names,
                       names_cap, names_n, base_off, name_off, off_cap, n_reads);
}

// TEST HOOK (include/g2s_test.h): the plan of the store route's capacities, on the host
int g2s_test_filter_store_plan(const void* bytes, size_t n, uint64_t* sample_records, uint64_t* sample_bytes,
                               uint64_t* sample_stored, uint64_t* rows_cap, uint64_t* store_cap, uint64_t* need) {
  if (!bytes) { g2s::set_filter_error("g2s_test_filter_store_plan: bad argument"); return G2S_ERR_ARG; }
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bytes, n, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  g2s::StorePlan p;
  if (!bam.store_sample(g2s::store_ask_from_env().sample, &p, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  if (sample_records) *sample_records = p.sample_records;
  if (sample_bytes) *sample_bytes = p.sample_bytes;
  if (sample_stored) *sample_stored = p.sample_stored;
  if (rows_cap) *rows_cap = p.rows_cap;
  if (store_cap) *store_cap = p.store_cap;
  if (need) *need = p.need;
  g2s::set_filter_error("");
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h): the store alone
int g2s_test_bam_store(const void* bytes, size_t n, int device, size_t window, uint8_t* store, uint64_t store_cap,
                       uint64_t* store_n, uint64_t* rec_off, uint64_t off_cap, uint64_t* n_records) {
  if (!bytes || !store_n || !n_records || (store_cap && !store) || (off_cap && !rec_off)) {
    g2s::set_filter_error("g2s_test_bam_store: bad argument");
    return G2S_ERR_ARG;
  }
  *store_n = *n_records = 0;
  if (device >= 0 && !g2s::filter_device_usable(device)) {
    g2s::set_filter_error("g2s_test_bam_store: no usable gfx950 device " + std::to_string(device));
    return G2S_ERR_NO_DEVICE;
  }
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bytes, n, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  bam.set_threads(1);
  bam.set_inflate_device(device >= 0 ? device : -1);
  std::vector<uint8_t> S;
  std::vector<uint64_t> off;
  if (device >= 0) {
    int anomaly = 0, refused = 0;
    g2s::BamFile::StoreAsk sa;  // (no switch is read: the store always, at the capacities that cannot overflow)
    sa.mode = 1;
    sa.worst_case = true;
    std::unique_ptr<g2s::BamRowsDevice> D = g2s::pass_a_device(bam, window, &anomaly, true, &refused, &sa);
    if (!D || !D->store_form()) {  // (never the host in the kernels' place)
      g2s::set_filter_error("g2s_test_bam_store: no store (anomaly " + std::to_string(anomaly) + ", refused " +
                            std::to_string(refused) + ")");
      return G2S_ERR_HIP;
    }
    if (!D->download_store(&S, &off, &err)) { g2s::set_filter_error(err); return G2S_ERR_HIP; }
  } else if (!bam.store_on_host(&S, &off, &err)) {
    g2s::set_filter_error(err);
    return G2S_ERR_IO;
  }
  *store_n = S.size();
  *n_records = off.size();
  if (store_cap && !S.empty()) memcpy(store, S.data(), (size_t)std::min<uint64_t>(store_cap, S.size()));
  if (off_cap && !off.empty()) memcpy(rec_off, off.data(), 8 * (size_t)std::min<uint64_t>(off_cap, off.size()));
  g2s::set_filter_error("");
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h)
int g2s_test_last_filter_store(int* used, uint64_t* records, uint64_t* store_bytes, uint64_t* store_cap, uint64_t* rows_cap,
                               uint64_t* device_bytes, int* overflow) {
  std::lock_guard<std::mutex> lk(g2s::g_last_mu);
  const g2s::StoreReport& r = g2s::g_last_store;
  if (used) *used = r.used;
  if (records) *records = r.records;
  if (store_bytes) *store_bytes = r.store_bytes;
  if (store_cap) *store_cap = r.store_cap;
  if (rows_cap) *rows_cap = r.rows_cap;
  if (device_bytes) *device_bytes = r.device_bytes;
  if (overflow) *overflow = r.overflow;
  return G2S_OK;
}

// pass A alone (g2s_test_bam_rows; `keep`: g2s_test_bam_rows_kept)
static int bam_rows_hook(bool keep, const void* bytes, size_t n, int device, size_t window, uint64_t cap, int32_t* ref_id,
                         int32_t* pos, int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate, uint64_t* total,
                         int32_t* read_length, int64_t* max_span) {
  if (!bytes || !total || !read_length || !max_span || (cap && (!ref_id || !pos || !end || !flag || !h_own || !h_mate))) {
    g2s::set_filter_error("g2s_test_bam_rows: bad argument");
    return G2S_ERR_ARG;
  }
  *total = 0;
  *read_length = 0;
  *max_span = 1;
  if (device >= 0 && !g2s::filter_device_usable(device)) {
    g2s::set_filter_error("g2s_test_bam_rows: no usable gfx950 device " + std::to_string(device));
    return G2S_ERR_NO_DEVICE;
  }
  g2s::BamFile bam;
  std::string err;
  if (!bam.open_mem(bytes, n, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  bam.set_threads(1);
  bam.set_inflate_device(device >= 0 ? device : -1);
  g2s::LastRows lr;
  auto note = [&] {
    std::lock_guard<std::mutex> lk(g2s::g_last_mu);
    g2s::g_last_rows = lr;
  };
  if (device >= 0) {
    int refused = 0;
    std::unique_ptr<g2s::BamRowsDevice> D = g2s::pass_a_device(bam, window, &lr.anomaly, keep, &refused);
    lr.windows = bam.rows_windows();
    if (D && keep && !D->stream_buffer()) {  // (never the two-slot route in the resident one's place)
      note();
      g2s::set_filter_error("g2s_test_bam_rows_kept: the stream was not kept (refused " + std::to_string(refused) + ")");
      return G2S_ERR_HIP;
    }
    if (!D) {  // (never the host in the kernels' place)
      note();
      g2s::set_filter_error("g2s_test_bam_rows: the device gave up its rows (anomaly " + std::to_string(lr.anomaly) + ")");
      return G2S_ERR_HIP;
    }
    const g2s::DeviceRows& R = D->rows();
    lr.on_device = 1;
    lr.records = R.n;
    lr.candidates = D->candidates();
    note();
    *total = R.n;
    *read_length = R.read_length;
    *max_span = R.max_span;
    if (!D->download(std::min<uint64_t>(cap, R.n), ref_id, pos, end, flag, h_own, h_mate, &err)) {
      g2s::set_filter_error(err);
      return G2S_ERR_HIP;
    }
    g2s::set_filter_error("");
    return G2S_OK;
  }
  g2s::FilterRows R;
  bool too_many = false;
  if (!g2s::pass_a_host(bam, R, read_length, &too_many, &err)) { g2s::set_filter_error(err); return G2S_ERR_IO; }
  if (too_many) { g2s::set_filter_error("more than 2^32 - 2 records"); return G2S_ERR_ARG; }
  lr.records = R.size();
  note();
  *total = R.size();
  *max_span = R.max_span;
  const size_t m = (size_t)std::min<uint64_t>(cap, R.size());
  if (m) {
    memcpy(ref_id, R.ref_id.data(), m * 4);
    memcpy(pos, R.pos.data(), m * 4);
    memcpy(end, R.end.data(), m * 8);
    memcpy(flag, R.flag.data(), m * 4);
    memcpy(h_own, R.h_own.data(), m * 8);
    memcpy(h_mate, R.h_mate.data(), m * 8);
  }
  g2s::set_filter_error("");
  return G2S_OK;
}

// TEST HOOKS (include/g2s_test.h)
int g2s_test_bam_rows(const void* bytes, size_t n, int device, size_t window, uint64_t cap, int32_t* ref_id, int32_t* pos,
                      int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate, uint64_t* total, int32_t* read_length,
                      int64_t* max_span) {
  return bam_rows_hook(false, bytes, n, device, window, cap, ref_id, pos, end, flag, h_own, h_mate, total, read_length, max_span);
}
int g2s_test_bam_rows_kept(const void* bytes, size_t n, int device, size_t window, uint64_t cap, int32_t* ref_id, int32_t* pos,
                           int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate, uint64_t* total,
                           int32_t* read_length, int64_t* max_span) {
  return bam_rows_hook(device >= 0, bytes, n, device, window, cap, ref_id, pos, end, flag, h_own, h_mate, total, read_length,
                       max_span);
}

// TEST HOOK (include/g2s_test.h)
int g2s_test_name_hash(const void* bytes, size_t len, int which, uint64_t* std_hash, uint64_t* own_hash) {
  if ((len && !bytes) || (which != 1 && which != 2) || !std_hash || !own_hash || len > 255) {
    g2s::set_filter_error("g2s_test_name_hash: bad argument");
    return G2S_ERR_ARG;
  }
  const size_t nlen = len ? strnlen((const char*)bytes, len) : 0;
  const std::string full = std::string((const char*)bytes, nlen) + (which == 1 ? "/1" : "/2");
  *std_hash = (uint64_t)std::hash<std::string>{}(full);
  *own_hash = g2s::name_hash((const uint8_t*)bytes, (uint32_t)nlen, (uint32_t)which);
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h)
int g2s_test_last_filter_rows(int* on_device, uint64_t* windows, uint64_t* records, uint64_t* candidates, int* anomaly) {
  std::lock_guard<std::mutex> lk(g2s::g_last_mu);
  if (on_device) *on_device = g2s::g_last_rows.on_device;
  if (windows) *windows = g2s::g_last_rows.windows;
  if (records) *records = g2s::g_last_rows.records;
  if (candidates) *candidates = g2s::g_last_rows.candidates;
  if (anomaly) *anomaly = g2s::g_last_rows.anomaly;
  return G2S_OK;
}

// TEST HOOK (include/g2s_test.h): one of the joins on the caller's rows and windows.  The path is the caller's
// choice alone: no G2S_HOST_FILTER, and a device that cannot run the kernels is an error, not the host path.
int g2s_test_filter_join(int device, int32_t threads, uint64_t nr, const int32_t* ref_id, const int32_t* pos,
                         const int64_t* end, const uint32_t* flag, const uint64_t* h_own, const uint64_t* h_mate,
                         int64_t max_span, uint64_t bits, uint64_t n, const int64_t* windows, uint64_t max_pairs,
                         uint64_t* list1, uint64_t cap1, uint64_t* n1, uint64_t* list2, uint64_t cap2, uint64_t* n2) {
  if ((nr && (!ref_id || !pos || !end || !flag || !h_own || !h_mate)) || (n && !windows) || !n1 || !n2 ||
      (cap1 && !list1) || (cap2 && !list2) || nr >= (uint64_t)UINT32_MAX - 1 || n > g2s::kFilterGapMask || threads < 1) {
    g2s::set_filter_error("g2s_test_filter_join: bad argument");
    return G2S_ERR_ARG;
  }
  *n1 = *n2 = 0;
  if (device >= 0 && !g2s::filter_device_usable(device)) {
    g2s::set_filter_error("g2s_test_filter_join: no usable gfx950 device " + std::to_string(device));
    return G2S_ERR_NO_DEVICE;
  }
  g2s::FilterRows R;
  R.ref_id.assign(ref_id, ref_id + nr);
  R.pos.assign(pos, pos + nr);
  R.end.assign(end, end + nr);
  R.flag.assign(flag, flag + nr);
  R.h_own.assign(h_own, h_own + nr);
  R.h_mate.assign(h_mate, h_mate + nr);
  R.max_span = max_span;
  g2s::FilterJoin J;
  J.rows = &R;
  J.bits = bits;
  J.max_pairs = max_pairs;
  J.win.resize(3 * (size_t)n);
  for (size_t i = 0; i < 3 * (size_t)n; i++)
    J.win[i] = g2s::FilterWindow{(int32_t)windows[3 * i], 0, windows[3 * i + 1], windows[3 * i + 2]};
  std::string err;
  const int rc = device >= 0 ? g2s::filter_join_device(J, device, &err) : g2s::filter_join_host(J, threads, &err);
  g2s::set_filter_error(err);
  if (rc != G2S_OK) return rc;
  *n1 = J.list1.size();
  *n2 = J.list2.size();
  if (cap1 && *n1) memcpy(list1, J.list1.data(), 8 * (size_t)std::min<uint64_t>(cap1, *n1));
  if (cap2 && *n2) memcpy(list2, J.list2.data(), 8 * (size_t)std::min<uint64_t>(cap2, *n2));
  return G2S_OK;
}

}  // extern "C"
