// gap2seq_amd/csrc/api_test_hooks.hip — the C ABI's test hooks (include/g2s_test.h) that need nothing of a session.
#include <algorithm>
#include <cstring>
#include <vector>

#include "api_internal.h"
#include "d3_device.h"
#include "fill_seg.h"
#include "glibc_rand.hpp"
#include "post.hpp"

using namespace g2s;
using namespace g2s::api;

// TEST HOOK (include/g2s_test.h)
extern "C" int g2s_test_seg_back_record(g2s_graph* g, int device, uint32_t node, uint32_t out[5]) {
  g2s_env_sync();
  if (!g || !out || (uint64_t)node >= 2 * g->g->n) return fail(G2S_ERR_ARG, "g2s_test_seg_back_record: bad argument");
  int rc = g2s_graph_upload(g, device);
  if (rc != G2S_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  rc = ensure_seg_tables(g, device);
  if (rc != G2S_OK) return rc;
  HIP_TRY(hipMemcpy(out, g->g->dev.at(device).back_table() + (size_t)(node ^ 1u) * 8, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return G2S_OK;
}

// TEST HOOK, see include/g2s_test.h: host half of phase D on a caller-supplied DP table.
// The closure the g2s_extract kernel would compute is derived on the host (host_closure).
extern "C" int g2s_test_post_gap(const g2s_graph* gh, const g2s_params* p, const g2s_gap* gap, int32_t n_states,
                                 const uint32_t* nodes, const int32_t* depths, const uint32_t* counts,
                                 int32_t c_count, int32_t n_lengths, const int32_t* lengths, int32_t reached_j,
                                 int32_t final_d, uint32_t seed, uint32_t skip, g2s_result* res, char* buf) {
  if (!gh || !p || !gap || !res || !buf || n_states < 0) return fail(G2S_ERR_ARG, "g2s_test_post_gap: bad argument");
  const Graph& g = *gh->g;
  const int k = g.k;
  GapJob j;
  j.g = gap->gap_len; j.lmf = gap->lmf; j.rmf = gap->rmf;
  if (gap->left_len < k + j.lmf || gap->right_len < k + j.rmf) return fail(G2S_ERR_ARG, "flank too short");
  std::vector<uint32_t> flank_store;
  j.resolve_on_host(g, gap->left, (size_t)gap->left_len, gap->right, (size_t)gap->right_len, &flank_store);
  HostTable t;
  t.D = j.lmf + j.rmf + j.g + p->d_err;
  t.lvl.assign((size_t)t.D + 2, 0);
  for (int i = 0; i < n_states; i++) if (depths[i] >= 0 && depths[i] <= t.D) t.lvl[(size_t)depths[i] + 1]++;
  for (int d = 0; d <= t.D; d++) t.lvl[(size_t)d + 1] += t.lvl[(size_t)d];
  t.states.assign((size_t)n_states + 1, 0);
  {
    std::vector<uint32_t> pos(t.lvl.begin(), t.lvl.end() - 1);
    for (int i = 0; i < n_states; i++)
      if (depths[i] >= 0 && depths[i] <= t.D)
        t.states[pos[(size_t)depths[i]]++] = ((uint64_t)nodes[i] << 32) | std::min<uint32_t>(counts[i], G2S_MAX_PATHS);
    for (int d = 0; d <= t.D; d++) std::sort(t.states.begin() + t.lvl[(size_t)d], t.states.begin() + t.lvl[(size_t)d + 1]);
  }
  GapOut go;
  memset(&go, 0, sizeof go);
  go.c_count = c_count; go.n_len = n_lengths; go.reached_j = reached_j; go.final_d = final_d;
  for (int i = 0; i < n_lengths && i < 2; i++) go.len[i] = lengths[i];
  FillParams fp;
  fp.k = k; fp.d_err = p->d_err; fp.skip_confident = p->skip_confident != 0; fp.all_paths = p->all_paths != 0;
  fp.unique_paths = p->unique_paths != 0;
  std::vector<SubState> closure;
  uint32_t q7 = 0;
  host_closure(g, fp, j, t, go, &closure, &q7);
  std::vector<SubRec> recs;
  std::vector<uint64_t> xps;
  sub_convert(closure.data(), (uint32_t)closure.size(), &recs, &xps);
  SubView v;
  v.out = &go; v.st = recs.data(); v.n = (uint32_t)recs.size(); v.xp = xps.data(); v.n_xp = (uint32_t)xps.size();
  SubPrep prep;
  sub_analyze(fp, j, v, &prep);
  memset(res, 0, sizeof *res);
  memset(buf, 0, j.buf_bytes(k, fp.d_err));
  res->phaseC_count = c_count;
  res->count = prep.count;
  res->flags |= prep.flags | q7;
  res->fill_off = (uint64_t)j.lmf;
  if (prep.phase_d) {
    GlibcRand rng;
    rng.seed(seed);
    for (uint32_t i = 0; i < skip; i++) rng.next();
    std::vector<uint32_t> rands((size_t)t.D + 4);
    for (auto& x : rands) x = (uint32_t)rng.next() << 1;  // raw words: value = word >> 1
    const int pick = (int)((rands[0] >> 1) % (uint32_t)go.n_len);
    const int fixed = sub_fixed_draws(v, prep, pick);
    sub_traceback(g, fp, j, v, prep, rands.data(), buf, res);
    if (fixed >= 0 && fixed != res->draws) return fail(G2S_ERR_STATE, "stop-depth analysis disagrees with the traceback");
    // the two shortcuts of the batch path, checked here on the CPU: the draw-count walk, and
    // the fill written without rand() values when no state has a second parent
    if (sub_count_draws(g, v, prep, rands.data()) != res->draws)
      return fail(G2S_ERR_STATE, "draw-count walk disagrees with the traceback");
    if (go.n_len == 1 && v.n_xp == 0 && fixed >= 0) {
      std::vector<char> buf2(j.buf_bytes(k, fp.d_err), 0);
      g2s_result r2;
      memset(&r2, 0, sizeof r2);
      sub_traceback(g, fp, j, v, prep, nullptr, buf2.data(), &r2);
      if (r2.draws != res->draws || r2.left_fuz != res->left_fuz || memcmp(buf2.data(), buf, buf2.size()) != 0)
        return fail(G2S_ERR_STATE, "rand()-free traceback disagrees with the traceback");
    }
    res->vertices = prep.sub[0]; res->edges = prep.sub[1]; res->nontrivial_components = prep.sub[2];
    res->size_nontrivial_components = prep.sub[3]; res->vertices_final = prep.sub[4]; res->edges_final = prep.sub[5];
    res->fill_off = (uint64_t)(j.lmf - res->left_fuz);
    res->fill_len = (int32_t)strlen(buf + res->fill_off);
  }
  return G2S_OK;
}

extern "C" int g2s_test_post_closure(const g2s_graph* gh, const g2s_params* p, const g2s_gap* gap, uint32_t n_records,
                                     const uint32_t* records, uint32_t n_xp, const uint64_t* xp, int32_t c_count,
                                     int32_t n_lengths, const int32_t* lengths, int32_t reached_j, int32_t final_d,
                                     uint32_t seed, uint64_t skip, g2s_result* res, char* buf) {
  if (!gh || !p || !gap || !res || !buf || (n_records && !records) || (n_xp && !xp))
    return fail(G2S_ERR_ARG, "g2s_test_post_closure: bad argument");
  const Graph& g = *gh->g;
  const int k = g.k;
  GapJob j;
  j.g = gap->gap_len; j.lmf = gap->lmf; j.rmf = gap->rmf;
  if (gap->left_len < k + j.lmf || gap->right_len < k + j.rmf) return fail(G2S_ERR_ARG, "flank too short");
  std::vector<uint32_t> flank_store;
  j.resolve_on_host(g, gap->left, (size_t)gap->left_len, gap->right, (size_t)gap->right_len, &flank_store);
  GapOut go;
  memset(&go, 0, sizeof go);
  go.c_count = c_count; go.n_len = n_lengths; go.reached_j = reached_j; go.final_d = final_d;
  for (int i = 0; i < n_lengths && i < 2; i++) go.len[i] = lengths[i];
  FillParams fp;
  fp.k = k; fp.d_err = p->d_err; fp.skip_confident = p->skip_confident != 0; fp.all_paths = p->all_paths != 0;
  fp.unique_paths = p->unique_paths != 0;
  std::vector<SubRec> recs(n_records);
  if (n_records) memcpy(recs.data(), records, (size_t)n_records * sizeof(SubRec));
  std::vector<uint64_t> xps(xp, xp + n_xp);
  std::sort(xps.begin(), xps.end());
  SubView v;
  v.out = &go; v.st = recs.data(); v.n = n_records; v.xp = xps.data(); v.n_xp = n_xp;
  SubPrep prep;
  sub_analyze(fp, j, v, &prep);
  memset(res, 0, sizeof *res);
  memset(buf, 0, j.buf_bytes(k, fp.d_err));
  res->phaseC_count = c_count;
  res->n_lengths = n_lengths;
  for (int i = 0; i < n_lengths && i < 2; i++) res->lengths[i] = lengths[i];
  res->count = prep.count;
  res->flags |= prep.flags;
  res->fill_off = (uint64_t)j.lmf;
  if (prep.phase_d) {
    GlibcRand rng;
    rng.seed(seed);
    for (uint64_t i = 0; i < skip; i++) rng.next();
    const int D = j.lmf + j.rmf + j.g + p->d_err;
    std::vector<uint32_t> rands((size_t)D + 4);
    for (auto& x : rands) x = (uint32_t)rng.next() << 1;  // raw words: value = word >> 1
    sub_traceback(g, fp, j, v, prep, rands.data(), buf, res);
    res->vertices = prep.sub[0]; res->edges = prep.sub[1]; res->nontrivial_components = prep.sub[2];
    res->size_nontrivial_components = prep.sub[3]; res->vertices_final = prep.sub[4]; res->edges_final = prep.sub[5];
    res->fill_off = (uint64_t)(j.lmf - res->left_fuz);
    res->fill_len = (int32_t)strlen(buf + res->fill_off);
  }
  return G2S_OK;
}

extern "C" int g2s_test_post_segments(const g2s_graph* gh, const g2s_params* p, const g2s_gap* gap, uint32_t n_segs,
                                      const uint32_t* segs, int32_t c_count, int32_t n_lengths, const int32_t* lengths,
                                      int32_t reached_j, int32_t final_d, uint32_t seed, uint64_t skip, g2s_result* res,
                                      char* buf, int32_t* on_segments) {
  if (!gh || !p || !gap || !res || !buf || (n_segs && !segs)) return fail(G2S_ERR_ARG, "g2s_test_post_segments: bad argument");
  const Graph& g = *gh->g;
  const int k = g.k;
  GapJob j;
  j.g = gap->gap_len; j.lmf = gap->lmf; j.rmf = gap->rmf;
  if (gap->left_len < k + j.lmf || gap->right_len < k + j.rmf) return fail(G2S_ERR_ARG, "flank too short");
  std::vector<uint32_t> flank_store;
  j.resolve_on_host(g, gap->left, (size_t)gap->left_len, gap->right, (size_t)gap->right_len, &flank_store);
  GapOut go;
  memset(&go, 0, sizeof go);
  go.c_count = c_count; go.n_len = n_lengths; go.reached_j = reached_j; go.final_d = final_d;
  for (int i = 0; i < n_lengths && i < 2; i++) go.len[i] = lengths[i];
  FillParams fp;
  fp.k = k; fp.d_err = p->d_err; fp.skip_confident = p->skip_confident != 0; fp.all_paths = p->all_paths != 0;
  fp.unique_paths = p->unique_paths != 0;
  SubView v;
  v.out = &go; v.segs = (const SegRec*)segs; v.n_segs = n_segs;
  SubPrep prep;
  const auto t_an0 = std::chrono::steady_clock::now();
  const bool ok = seg_analyze(fp, j, v, &prep);
  if (on_segments) *on_segments = ok ? 1 : 0;
  if (n_segs >= 2000 && prep.run_mode && GENV("G2S_POST_LAPS")) {  // (tools/host_items_replay.py)
    const double* l = g2s_post_laps;
    const double t1 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    fprintf(stderr, "[g2s] %u segments, run analysis laps (us): front %.0f | collect %.0f merge+sort %.0f runs %.0f edges %.0f csr %.0f tarjan %.0f rest %.0f | all %.0f\n", n_segs,
            l[0] - std::chrono::duration<double, std::micro>(t_an0.time_since_epoch()).count(), l[1] - l[0], l[2] - l[1], l[3] - l[2], l[4] - l[3], l[5] - l[4], l[6] - l[5], l[7] - l[6],
            t1 - std::chrono::duration<double, std::micro>(t_an0.time_since_epoch()).count());
  }
  memset(res, 0, sizeof *res);
  memset(buf, 0, j.buf_bytes(k, fp.d_err));
  if (!ok) return G2S_OK;  // a k-mer at two depths: the caller takes g2s_test_seg_expand + g2s_test_post_closure
  res->phaseC_count = c_count;
  res->n_lengths = n_lengths;
  for (int i = 0; i < n_lengths && i < 2; i++) res->lengths[i] = lengths[i];
  res->count = prep.count;
  res->flags |= prep.flags;
  res->fill_off = (uint64_t)j.lmf;
  if (prep.phase_d) {
    GlibcRand rng;
    rng.seed(seed);
    for (uint64_t i = 0; i < skip; i++) rng.next();
    const int D = j.lmf + j.rmf + j.g + p->d_err;
    std::vector<uint32_t> rands((size_t)D + 4);
    for (auto& x : rands) x = (uint32_t)rng.next() << 1;
    const int pick = (int)((rands[0] >> 1) % (uint32_t)go.n_len);
    const int fixed = sub_fixed_draws(v, prep, pick);
    seg_traceback(g, fp, j, v, prep, rands.data(), buf, res);
    if (fixed >= 0 && fixed != res->draws) return fail(G2S_ERR_STATE, "stop-depth analysis disagrees with the traceback (segments)");
    if (seg_count_draws(g, v, prep, rands.data()) != res->draws)
      return fail(G2S_ERR_STATE, "draw-count walk disagrees with the traceback (segments)");
    if (go.n_len == 1 && !prep.has_choice && fixed >= 0) {
      std::vector<char> buf2(j.buf_bytes(k, fp.d_err), 0);
      g2s_result r2;
      memset(&r2, 0, sizeof r2);
      seg_traceback(g, fp, j, v, prep, nullptr, buf2.data(), &r2);
      if (r2.draws != res->draws || r2.left_fuz != res->left_fuz || memcmp(buf2.data(), buf, buf2.size()) != 0)
        return fail(G2S_ERR_STATE, "rand()-free traceback disagrees with the traceback (segments)");
    }
    res->vertices = prep.sub[0]; res->edges = prep.sub[1]; res->nontrivial_components = prep.sub[2];
    res->size_nontrivial_components = prep.sub[3]; res->vertices_final = prep.sub[4]; res->edges_final = prep.sub[5];
    res->fill_off = (uint64_t)(j.lmf - res->left_fuz);
    res->fill_len = (int32_t)strlen(buf + res->fill_off);
  }
  return G2S_OK;
}

extern "C" int g2s_test_seg_expand(const g2s_graph* gh, const g2s_params* p, const g2s_gap* gap, uint32_t n_segs,
                                   const uint32_t* segs, int32_t n_lengths, const int32_t* lengths, int32_t reached_j,
                                   uint32_t n_records, uint32_t* records, uint32_t n_xp, uint64_t* xp) {
  if (!gh || !p || !gap || (n_segs && !segs) || (n_records && !records) || (n_xp && !xp))
    return fail(G2S_ERR_ARG, "g2s_test_seg_expand: bad argument");
  const Graph& g = *gh->g;
  const int k = g.k;
  GapJob j;
  j.g = gap->gap_len; j.lmf = gap->lmf; j.rmf = gap->rmf;
  if (gap->left_len < k + j.lmf || gap->right_len < k + j.rmf) return fail(G2S_ERR_ARG, "flank too short");
  std::vector<uint32_t> flank_store;
  j.resolve_on_host(g, gap->left, (size_t)gap->left_len, gap->right, (size_t)gap->right_len, &flank_store);
  GapOut go;
  memset(&go, 0, sizeof go);
  go.n_len = n_lengths; go.reached_j = reached_j;
  for (int i = 0; i < n_lengths && i < 2; i++) go.len[i] = lengths[i];
  FillParams fp;
  fp.k = k; fp.d_err = p->d_err; fp.skip_confident = p->skip_confident != 0; fp.all_paths = p->all_paths != 0;
  fp.unique_paths = p->unique_paths != 0;
  const SegRec* sr = (const SegRec*)segs;
  size_t total = 0, nx = 0;
  for (uint32_t i = 0; i < n_segs; i++) {
    total += sr[i].depth_len >> 16;
    if (!(sr[i].flags & G2S_SUB_SOURCE)) {
      int np = ((sr[i].par01 & 0xFFFFu) != 0xFFFFu) + ((sr[i].par01 >> 16) != 0xFFFFu) + ((sr[i].par23 & 0xFFFFu) != 0xFFFFu) +
               ((sr[i].par23 >> 16) != 0xFFFFu);
      if (np > 1) nx += (size_t)np - 1;
    }
  }
  if (total != n_records || nx != n_xp) return fail(G2S_ERR_ARG, "g2s_test_seg_expand: output sizes do not match the segments");
  seg_expand(fp, j, go, sr, n_segs, (SubRec*)records, xp);
  return G2S_OK;
}

extern "C" int g2s_test_graph_tables(const g2s_graph* gh, uint32_t* succ_out, uint64_t* ustart_out) {
  if (!gh || !gh->g) return fail(G2S_ERR_ARG, "g2s_test_graph_tables: bad argument");
  const Graph& g = *gh->g;
  if (succ_out) memcpy(succ_out, g.succ.data(), (size_t)g.n * 8 * sizeof(uint32_t));
  if (ustart_out) memcpy(ustart_out, g.ustart.data(), (size_t)((g.n + 63) / 64) * 8);
  return G2S_OK;
}

extern "C" int g2s_test_device_rand(int device, uint32_t seed, uint64_t skip, uint32_t n, int32_t* out) {
  if (!out) return fail(G2S_ERR_ARG, "g2s_test_device_rand: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(G2S_ERR_NO_DEVICE, "no such device");
  HIP_TRY(hipSetDevice(device));
  GlibcRandStream st;
  st.seed(seed);
  for (uint64_t left = skip; left;) {  // the host's generator up to the position, as a session would have consumed it
    const size_t c = (size_t)std::min<uint64_t>(left, 1u << 20);
    st.ensure(c);
    st.consume(c);
    left -= c;
  }
  std::vector<uint32_t> tables((128 + 256 + 64) * 31);
  rand_tables_host(tables.data(), tables.data() + 128 * 31, tables.data() + (128 + 256) * 31);
  const uint64_t cap = ((uint64_t)n + 2 * G2S_RAND_BLOCK) & ~(uint64_t)(G2S_RAND_BLOCK - 1);
  uint32_t *d_tab = nullptr, *d_rnd = nullptr;
  D3Summary* d_sum = nullptr;
  HIP_TRY(hipMalloc((void**)&d_tab, tables.size() * 4));
  HIP_TRY(hipMalloc((void**)&d_rnd, (31 + cap + 64) * 4));
  HIP_TRY(hipMalloc((void**)&d_sum, sizeof(D3Summary)));
  D3Summary sum;
  memset(&sum, 0, sizeof sum);
  sum.draws_min = n;
  HIP_TRY(hipMemcpy(d_tab, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_sum, &sum, sizeof sum, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_rnd, st.window(G2S_RAND_WINDOW), G2S_RAND_WINDOW * 4, hipMemcpyHostToDevice));
  RandTables rt;
  rt.hi = d_tab; rt.mid = d_tab + 128 * 31; rt.lane = d_tab + (128 + 256) * 31;
  HIP_TRY(launch_rand_fill(nullptr, d_rnd, rt, d_sum, cap));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint32_t> h(n);
  HIP_TRY(hipMemcpy(h.data(), d_rnd + 31, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) out[i] = (int32_t)(h[i] >> 1);
  (void)hipFree(d_tab); (void)hipFree(d_rnd); (void)hipFree(d_sum);
  return G2S_OK;
}

// TEST HOOK: g2s_d3_tables_waves for one gap of the caller's design (d3_device.h: test_d3_tables)
extern "C" int g2s_test_d3_tables(int device, const uint32_t* segs, uint32_t n_segs, int32_t n_len, int32_t len0, int32_t len1,
                                  uint32_t start_seg, const uint32_t* rnd, uint64_t rnd_cap, uint32_t base, uint32_t R, uint32_t dmin,
                                  uint32_t dspread, uint16_t* entries, uint8_t* bad, uint32_t* anomalies) {
  if ((!segs && n_segs) || (!rnd && rnd_cap) || !entries || !bad || !anomalies || n_segs > 0xFFFFu || n_len < 1 || n_len > 2 ||
      (uint64_t)R + 1u > (uint64_t)G2S_D3_TABLE_BUDGET)
    return fail(G2S_ERR_ARG, "g2s_test_d3_tables: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(G2S_ERR_NO_DEVICE, "no such device");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(test_d3_tables(segs, n_segs, n_len, len0, len1, start_seg, rnd, rnd_cap, base, R, dmin, dspread, entries, bad, anomalies));
  return G2S_OK;
}

// TEST HOOK: lists of this process that took phase D3's short route (d3_device.h: d3_chain_launches)
extern "C" uint64_t g2s_test_d3_chain_launches(void) { return d3_chain_launches(); }

// TEST HOOK: the n values behind `skip` values that were drawn elsewhere — GlibcRandStream::skip, the jump by the
// recurrence's polynomial g2s_share_end moves a rank's generator with — for comparison with g2s_test_rand_stream
extern "C" int g2s_test_rand_skip(uint32_t seed, uint64_t skip, uint32_t n, int32_t* out) {
  if (!out) return fail(G2S_ERR_ARG, "g2s_test_rand_skip: bad argument");
  GlibcRandStream st;
  st.seed(seed);
  st.skip(skip);
  st.ensure(n);
  for (uint32_t i = 0; i < n; i++) out[i] = st.value(i);
  return G2S_OK;
}
extern "C" int g2s_test_rand_stream(uint32_t seed, uint32_t skip, uint32_t n, int32_t* out) {
  if (!out) return fail(G2S_ERR_ARG, "g2s_test_rand_stream: bad argument");
  GlibcRandStream st;
  st.seed(seed);
  // consume in two pieces so that the compaction path is exercised too
  st.ensure(skip / 2 + 1);
  st.consume(skip / 2);
  st.ensure(skip - skip / 2 + n);
  st.consume(skip - skip / 2);
  for (uint32_t i = 0; i < n; i++) out[i] = st.value(i);
  return G2S_OK;
}
