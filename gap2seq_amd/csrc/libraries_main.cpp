// gap2seq_amd/csrc/libraries_main.cpp — `Gap2Seq-libraries`: the wrapper's libraries flow (Gap2Seq.py -l,
// /root/reference/src/Gap2Seq.py:133-218) in one process.  For every gap the wrapper extracts the reads of every library
// that can belong to it (ReadFilter), adds every library's unmapped reads when too few bases came out, and runs a fresh
// Gap2Seq-core over those reads alone.  Here every library's reads are extracted for all gaps at once, with its unmapped
// reads, in two passes over its BAM, as a pool that holds every read once (g2s_filter_reads_gaps_pool: gap i's reads are
// g2s_filter_reads' for gap i); every gap's reads become one read set of a set graph built from the pools
// (g2s_graph_build_pool: a gap's own reads as indices, the unmapped reads as the list every gap under the threshold
// shares, encoded and sorted once a chunk) and the gaps are filled as one list (g2s_fill_sets): every gap's fill is
// what its own Gap2Seq-core -reads S(i) -left L -right R -length G run writes.  No FASTA text is formed.
//
//   Gap2Seq-libraries -libraries libs.txt -gaps gaps.fa -bed gaps.bed -filled out.fa
//                     [-k 31] [-fuz 10] [-solid 2] [-dist-error 500] [-max-mem 20] [-randseed 0]
//                     [-all-upper] [-unique] [-best-only] [-device D] [-filter-device D|-1] [-filter-one-pass 0|1]
//                     [-device-pool 0|1]
//
// -filter-device: the GPU the read filter's joins run on (default: -device), -1 = host threads.
// -filter-one-pass: 1 asks the read filter to inflate every BAM once and keep it on the GPU between its passes
// (g2s_filter_set_one_pass), 0 forbids it; not given, G2S_FILTER_ONE_PASS decides, and without that the mode is on
// (kOnePassDefault: DESIGN 3.6b has the measurement behind it).  A BAM too large to stay there whole keeps every
// record's head, name and bases instead (the store route, bam_store.h).  The output is the same bytes either way.
// -device-pool: 1 leaves every library's reads where the filter made them — in device memory when it ran one pass
// (g2s_filter_reads_gaps_dpool) — and builds every chunk's set graph from there (g2s_graph_build_dpool_reach): the reads
// never become host memory; 0 takes them through host memory (g2s_filter_reads_gaps_pool, g2s_graph_build_pool_reach).
// Not given, G2S_DEVICE_POOL=1|0 decides, and without that the switch is on (kDevicePoolDefault: DESIGN 3.6b).  With -filter-device different from -device the pools lie on another device and the
// build packs them on the host.  The output is the same bytes either way.
// libs.txt: tab separated `bam mean std_dev threshold`, one library a line.  out.fa: per gap, in input order,
// `comment\nfill\n` (the file GapMerger -gaps takes); stdout ends with `Filled X out of Y gaps`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/g2s.h"
#include "fastx.hpp"

namespace {

// Whether the libraries' BAM files are filtered in one-pass mode when neither -filter-one-pass nor G2S_FILTER_ONE_PASS
// says otherwise.  By DESIGN 3.6b's table the whole filter call in one-pass mode beats the parent's on average by
// more than the parent's own spread over six calls, with 8 and with 2 host threads.
constexpr bool kOnePassDefault = true;

// Whether the libraries' reads go from the filter to the set build as device-held pools when neither -device-pool nor
// G2S_DEVICE_POOL says otherwise.  By DESIGN 3.6b's table the way from a BAM file to its uploaded set graph through a
// device-held pool is 9 to 10 ms shorter on average than through host memory, on a 3 MB and on a 32 MB file, the two
// variants' ranges over six alternating calls disjoint at both sizes.
constexpr bool kDevicePoolDefault = true;

struct Library {
  std::string bam;
  int mean = 0, sd = 0;
  double threshold = 0;
};

struct GapRec {
  std::string comment, left, right, scaffold;
  int gap_length = 0, flank_length = 0, breakpoint = 0;
};

// parse_gap (Gap2Seq.py:246-262): left up to the first N/n, right after the last one
GapRec parse_gap(const std::string& record, const std::string& bed_line) {
  GapRec g;
  const size_t nl = record.find('\n');
  g.comment = record.substr(0, nl);
  std::string seq;
  if (nl != std::string::npos)
    for (size_t i = nl + 1; i < record.size(); i++)
      if (record[i] != '\n') seq += record[i];
  const size_t first = seq.find_first_of("Nn"), last = seq.find_last_of("Nn");
  g.left = first == std::string::npos ? seq.substr(0, seq.size() ? seq.size() - 1 : 0) : seq.substr(0, first);  // (find -1)
  g.right = last == std::string::npos ? seq : seq.substr(last + 1);
  g.flank_length = (int)std::min(g.left.size(), g.right.size());
  g.gap_length = (int)seq.size() - (int)g.left.size() - (int)g.right.size();
  std::vector<std::string> cols;
  std::stringstream ss(bed_line);
  std::string c;
  while (std::getline(ss, c, '\t')) cols.push_back(c);
  g.scaffold = cols.size() > 0 ? cols[0] : "";
  g.breakpoint = (cols.size() > 1 ? atoi(cols[1].c_str()) : 0) + (int)g.left.size();
  return g;
}

// the gap records of the gaps file as the wrapper cuts them (Gap2Seq.py:284-294): a new record at every '>' line
std::vector<std::string> gap_records(const std::string& text) {
  std::vector<std::string> out;
  std::string cur;
  size_t p = 0;
  while (p < text.size()) {
    size_t e = text.find('\n', p);
    e = e == std::string::npos ? text.size() : e + 1;
    const std::string line = text.substr(p, e - p);
    if (!line.empty() && line[0] == '>' && !cur.empty()) { out.push_back(cur); cur.clear(); }
    cur += line;
    p = e;
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

// the reads of every gap from one library, and the library's unmapped reads, in one call (two passes over the BAM), as
// a pool: every read held once however many gaps select it, every gap a list of indices.  A library whose BAM cannot
// be read gives no reads (as the wrapper's ReadFilter run that fails, Gap2Seq.py:151-153).
// (dpool: the pool as a g2s_device_pool in *dout, and its view returned)
const g2s_read_pool* filter_library(const Library& lib, const std::vector<GapRec>& gaps, int device, g2s_read_pool** hout,
                                    g2s_device_pool** dout) {
  g2s_filter_opts o;
  memset(&o, 0, sizeof o);
  o.mean_insert = lib.mean;
  o.std_dev = lib.sd;
  std::vector<g2s_filter_gap> gv(gaps.size());
  for (size_t i = 0; i < gaps.size(); i++) {
    gv[i].scaffold = gaps[i].scaffold.c_str();
    gv[i].breakpoint = gaps[i].breakpoint;
    gv[i].gap_length = gaps[i].gap_length;
    gv[i].flank_length = gaps[i].flank_length;
  }
  int64_t total = 0;
  // (with names: the chunk rule below counts the bytes of the FASTA text the reads would make; a device pool's view has
  // the names' lengths always)
  auto call = [&](int dev) {
    return dout ? g2s_filter_reads_gaps_dpool(lib.bam.c_str(), &o, gv.data(), gv.size(), dev, 1, dout, &total, nullptr)
                : g2s_filter_reads_gaps_pool(lib.bam.c_str(), &o, gv.data(), gv.size(), dev, 1, 1, hout, &total, nullptr);
  };
  int rc = call(device);
  if (rc != G2S_OK && rc != G2S_ERR_IO && device >= 0) {  // (the device could not take it: the same joins on the host)
    std::cerr << "Gap2Seq-libraries: " << lib.bam << ": " << g2s_filter_last_error() << "; filtering on the host" << std::endl;
    rc = call(-1);
  }
  if (rc != G2S_OK) {
    std::cerr << "Gap2Seq-libraries: " << lib.bam << ": " << g2s_filter_last_error() << std::endl;
    return nullptr;
  }
  return dout ? g2s_device_pool_view(*dout) : *hout;
}

}  // namespace

int main(int argc, char** argv) {
  std::string libs_path, gaps_path, bed_path, filled_path;
  int k = 31, fuz = 10, solid = 2, derr = 500, device = 0, filter_device = 0;
  bool filter_device_set = false;
  int filter_one_pass = -1, device_pool = -1;
  double max_mem = 20;
  uint32_t randseed = 0;
  bool upper = false, unique = false, best = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
    if (a == "-libraries") libs_path = val();
    else if (a == "-gaps") gaps_path = val();
    else if (a == "-bed") bed_path = val();
    else if (a == "-filled") filled_path = val();
    else if (a == "-k") k = atoi(val());
    else if (a == "-fuz") fuz = atoi(val());
    else if (a == "-solid") solid = atoi(val());
    else if (a == "-dist-error") derr = atoi(val());
    else if (a == "-max-mem") max_mem = atof(val());
    else if (a == "-randseed") randseed = (uint32_t)strtoul(val(), nullptr, 10);
    else if (a == "-device") device = atoi(val());
    else if (a == "-filter-device") { filter_device = atoi(val()); filter_device_set = true; }
    else if (a == "-filter-one-pass") filter_one_pass = atoi(val()) != 0 ? 1 : 0;
    else if (a == "-device-pool") device_pool = atoi(val()) != 0 ? 1 : 0;
    else if (a == "-all-upper") upper = true;
    else if (a == "-unique") unique = true;
    else if (a == "-best-only") best = true;
    else { std::cerr << "Gap2Seq-libraries: unknown parameter '" << a << "'" << std::endl; return EXIT_FAILURE; }
  }
  if (filter_one_pass < 0 && kOnePassDefault && !getenv("G2S_FILTER_ONE_PASS")) filter_one_pass = 1;
  g2s_filter_set_one_pass(filter_one_pass);
  if (device_pool < 0) {
    const char* e = getenv("G2S_DEVICE_POOL");
    device_pool = e ? (atoi(e) != 0 ? 1 : 0) : (kDevicePoolDefault ? 1 : 0);
  }
  if (libs_path.empty() || gaps_path.empty() || bed_path.empty() || filled_path.empty()) {
    std::cerr << "Gap2Seq-libraries: -libraries, -gaps, -bed and -filled are required" << std::endl;
    return EXIT_FAILURE;
  }
  std::string libs_text, gaps_text, bed_text;
  if (!g2s::read_text_file(libs_path, &libs_text) || !g2s::read_text_file(gaps_path, &gaps_text) ||
      !g2s::read_text_file(bed_path, &bed_text)) {
    std::cerr << "Gap2Seq-libraries: cannot read the input files" << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<Library> libs;
  {
    std::stringstream ls(libs_text);
    std::string line;
    while (std::getline(ls, line)) {
      if (line.empty()) continue;
      std::vector<std::string> cols;
      std::stringstream cs(line);
      std::string c;
      while (std::getline(cs, c, '\t')) cols.push_back(c);
      if (cols.size() < 4) { std::cerr << "Gap2Seq-libraries: a library line needs bam, mean, std_dev, threshold" << std::endl; return EXIT_FAILURE; }
      Library L;
      L.bam = cols[0];
      L.mean = atoi(cols[1].c_str());
      L.sd = atoi(cols[2].c_str());
      L.threshold = atof(cols[3].c_str());
      libs.push_back(L);
    }
  }
  const std::vector<std::string> records = gap_records(gaps_text);
  std::vector<std::string> bed_lines;
  {
    std::stringstream bs(bed_text);
    std::string line;
    while (std::getline(bs, line)) bed_lines.push_back(line);
  }
  const size_t ngaps = records.size();
  std::vector<GapRec> gaps(ngaps);
  for (size_t i = 0; i < ngaps; i++) gaps[i] = parse_gap(records[i], i < bed_lines.size() ? bed_lines[i] : std::string());
  // ---- every library's pool; the reads of all libraries as one array of (pointer, length), every gap's own list
  // (its reads of library 0, 1, ... in order) as indices into it, and the shared list: every library's unmapped reads
  // in library order.  What is held is the pools and the index lists: nothing grows with gaps x unmapped reads.
  std::vector<const g2s_read_pool*> pools;  // (a library's arrays: its host pool, or the view of its device pool)
  std::vector<g2s_read_pool*> host_pools;
  std::vector<g2s_device_pool*> dev_pools;  // (-device-pool 1: the libraries that gave reads, in order)
  std::vector<const char*> seq_ptr;         // (null for a read of a device pool)
  std::vector<uint64_t> seq_len, seq_fasta;  // (bytes of the read's FASTA record: '>' name '\n' bases '\n')
  std::vector<uint32_t> lib_first;
  double threshold = 0;
  for (const Library& L : libs) {  // (Gap2Seq.py:143-159; every library's unmapped reads, Gap2Seq.py:64-72, :437-439)
    g2s_read_pool* hp = nullptr;
    g2s_device_pool* dp = nullptr;
    const g2s_read_pool* P = filter_library(L, gaps, filter_device_set ? filter_device : device, &hp, device_pool ? &dp : nullptr);
    pools.push_back(P);
    if (hp) host_pools.push_back(hp);
    if (dp) dev_pools.push_back(dp);
    lib_first.push_back((uint32_t)seq_ptr.size());
    if (P) {
      if (seq_ptr.size() + P->n_reads >= ((uint64_t)1 << 32)) { std::cerr << "Gap2Seq-libraries: 2^32 reads or more selected" << std::endl; return EXIT_FAILURE; }
      for (uint64_t r = 0; r < P->n_reads; r++) {
        seq_ptr.push_back(P->bases ? P->bases + P->base_off[r] : nullptr);
        seq_len.push_back(P->base_off[r + 1] - P->base_off[r]);
        seq_fasta.push_back(seq_len.back() + (P->name_off[r + 1] - P->name_off[r]) + 3);
      }
    }
    threshold += L.threshold;
  }
  if (device_pool && getenv("G2S_DEBUG")) {
    size_t held = 0;
    uint64_t bytes = 0;
    for (const g2s_device_pool* P : dev_pools) {
      held += g2s_device_pool_device(P) >= 0 ? 1 : 0;
      bytes += g2s_device_pool_bytes(P);
    }
    std::cerr << "[g2s] libraries: " << held << " of " << dev_pools.size() << " pools held on the device (" << bytes << " bytes)"
              << std::endl;
  }
  std::vector<uint64_t> own_begin(ngaps + 1, 0);
  for (size_t i = 0; i < ngaps; i++) {
    own_begin[i + 1] = own_begin[i];
    for (const g2s_read_pool* P : pools)
      if (P) own_begin[i + 1] += P->gap_begin[i + 1] - P->gap_begin[i];
  }
  std::vector<uint32_t> own_seq((size_t)own_begin[ngaps]), shared_seq;
  std::vector<size_t> filtered_length(ngaps, 0), text_bytes(ngaps, 0);  // (text_bytes: of the gap's reads as FASTA text)
  size_t shared_bytes = 0;
  for (size_t l = 0; l < pools.size(); l++) {
    if (!pools[l]) continue;
    for (uint64_t q = 0; q < pools[l]->n_unmapped; q++) {
      shared_seq.push_back(lib_first[l] + pools[l]->unmapped_read[q]);
      shared_bytes += (size_t)seq_fasta[shared_seq.back()];
    }
  }
  for (size_t i = 0; i < ngaps; i++) {
    size_t o = (size_t)own_begin[i];
    for (size_t l = 0; l < pools.size(); l++) {
      if (!pools[l]) continue;
      for (uint64_t q = pools[l]->gap_begin[i]; q < pools[l]->gap_begin[i + 1]; q++) {
        const uint32_t j = lib_first[l] + pools[l]->gap_read[q];
        own_seq[o++] = j;
        // `grep '^[^>;]' file | wc -c` (Gap2Seq.py:156-159) on the FASTA text of these reads: every sequence line with its
        // newline; a read without bases leaves an empty line, which the pattern does not match
        if (seq_len[j]) filtered_length[i] += (size_t)seq_len[j] + 1;
        text_bytes[i] += (size_t)seq_fasta[j];
      }
    }
  }
  std::vector<uint8_t> takes_unmapped(ngaps, 0);
  for (size_t i = 0; i < ngaps; i++) {
    const GapRec& g = gaps[i];
    const double ratio = g.gap_length > 0 ? (double)filtered_length[i] / (double)g.gap_length : INFINITY;
    if (ratio < threshold) {  // (Gap2Seq.py:161-167)
      takes_unmapped[i] = 1;
      text_bytes[i] += shared_bytes;
    }
  }
  // ---- fill: chunks of gaps whose read text fits a budget, one set graph and one list each
  g2s_params p;
  memset(&p, 0, sizeof p);
  p.d_err = derr;
  p.skip_confident = upper ? 1 : 0;
  p.all_paths = best ? 0 : 1;
  p.unique_paths = unique ? 1 : 0;
  p.max_mem = (int64_t)(max_mem * 1024.0 * 1024.0 * 1024.0);  // (the wrapper's per-gap core runs with -nb-cores 1)
  p.randseed = randseed;
  std::vector<std::string> fills(ngaps);
  const size_t budget = (size_t)256 << 20;
  std::vector<uint32_t> chunk_of(seq_ptr.size(), UINT32_MAX), touched;  // a read's index in the chunk being built
  size_t lo = 0;
  while (lo < ngaps) {
    size_t hi = lo, bytes = 0;
    while (hi < ngaps && (hi == lo || bytes + text_bytes[hi] <= budget)) bytes += text_bytes[hi++];
    // the chunk's sets over the reads the chunk names: indices rebased to the chunk, no text moves
    std::vector<const char*> sp;
    std::vector<uint64_t> sl, set_begin(1, 0);
    std::vector<uint32_t> set_seq, chunk_shared;
    auto local = [&](uint32_t j) -> uint32_t {
      if (device_pool) return j;  // (the build numbers the pools' reads as lib_first does: nothing to rebase)
      if (chunk_of[j] == UINT32_MAX) { chunk_of[j] = (uint32_t)sp.size(); sp.push_back(seq_ptr[j]); sl.push_back(seq_len[j]); touched.push_back(j); }
      return chunk_of[j];
    };
    bool any_shared = false;
    for (size_t i = lo; i < hi; i++) {
      for (uint64_t q = own_begin[i]; q < own_begin[i + 1]; q++) set_seq.push_back(local(own_seq[(size_t)q]));
      set_begin.push_back(set_seq.size());
      any_shared = any_shared || takes_unmapped[i];
    }
    if (any_shared)
      for (uint32_t j : shared_seq) chunk_shared.push_back(local(j));
    // every gap's set bounded to what its fill can reach (g2s_graph_build_pool_reach: the sound radius); a gap that is
    // not filled (a flank shorter than k) gets an empty set.  G2S_NO_REACH=1: the whole sets.
    std::vector<g2s_gap> reach_gap(hi - lo);
    std::vector<int32_t> reach_radius(hi - lo, -1);
    const bool use_reach = !(getenv("G2S_NO_REACH") && atoi(getenv("G2S_NO_REACH")) != 0);
    for (size_t i = lo; use_reach && i < hi; i++) {
      const GapRec& g = gaps[i];
      g2s_gap& x = reach_gap[i - lo];
      memset(&x, 0, sizeof x);
      x.left = g.left.c_str();
      x.right = g.right.c_str();
      x.left_len = (int)g.left.size();
      x.right_len = (int)g.right.size();
      x.gap_len = g.gap_length;
      x.lmf = std::min((int)g.left.size() - k, fuz);   // (negative for a flank shorter than k: no seeds, an empty set)
      x.rmf = std::min((int)g.right.size() - k, fuz);
      x.skip_if_prev_right_fuz_gt = -1;
      reach_radius[i - lo] = std::max(0, g.gap_length + derr) + std::max(0, x.lmf) + std::max(0, x.rmf);
    }
    g2s_graph* graph = nullptr;
    int rc;
    if (device_pool && dev_pools.empty()) {  // (no library gave reads: the build over no sequences)
      rc = g2s_graph_build_pool_reach(nullptr, nullptr, 0, set_begin.data(), set_seq.data(), chunk_shared.data(), chunk_shared.size(),
                                      takes_unmapped.data() + lo, (uint32_t)(hi - lo), k, solid, 0,
                                      use_reach ? reach_gap.data() : nullptr, use_reach ? reach_radius.data() : nullptr, &graph);
    } else if (device_pool) {
      rc = g2s_graph_build_dpool_reach(dev_pools.data(), (uint32_t)dev_pools.size(), set_begin.data(), set_seq.data(),
                                       chunk_shared.data(), chunk_shared.size(), takes_unmapped.data() + lo, (uint32_t)(hi - lo), k,
                                       solid, 0, use_reach ? reach_gap.data() : nullptr, use_reach ? reach_radius.data() : nullptr,
                                       &graph);
    } else {
      rc = g2s_graph_build_pool_reach(sp.data(), sl.data(), sp.size(), set_begin.data(), set_seq.data(), chunk_shared.data(),
                                      chunk_shared.size(), takes_unmapped.data() + lo, (uint32_t)(hi - lo), k, solid, 0,
                                      use_reach ? reach_gap.data() : nullptr, use_reach ? reach_radius.data() : nullptr, &graph);
    }
    for (uint32_t j : touched) chunk_of[j] = UINT32_MAX;
    touched.clear();
    g2s_session* s = nullptr;
    if (rc == G2S_OK) rc = g2s_session_create(graph, device, &p, &s);
    if (rc != G2S_OK) {
      std::cerr << "Gap2Seq-libraries: " << g2s_last_error() << std::endl;
      if (graph) g2s_graph_free(graph);
      return EXIT_FAILURE;
    }
    std::vector<g2s_gap> gv;
    std::vector<uint32_t> gs, idx;
    for (size_t i = lo; i < hi; i++) {
      const GapRec& g = gaps[i];
      if ((int)g.left.size() < k || (int)g.right.size() < k) continue;  // Gap2Seq-core writes nothing (Gap2Seq.cpp:233-236)
      g2s_gap x;
      memset(&x, 0, sizeof x);
      x.left = g.left.c_str();
      x.right = g.right.c_str();
      x.left_len = (int)g.left.size();
      x.right_len = (int)g.right.size();
      x.gap_len = g.gap_length;
      x.lmf = std::min((int)g.left.size() - k, fuz);
      x.rmf = std::min((int)g.right.size() - k, fuz);
      x.skip_if_prev_right_fuz_gt = -1;
      gv.push_back(x);
      gs.push_back((uint32_t)(i - lo));
      idx.push_back((uint32_t)i);
    }
    size_t arena_bytes = 0;
    for (const g2s_gap& x : gv) arena_bytes += (size_t)(std::max(0, x.gap_len) + k + derr + x.lmf + x.rmf + 3);
    std::vector<char> arena(std::max<size_t>(arena_bytes, 1));
    std::vector<g2s_result> res(std::max<size_t>(gv.size(), 1));
    rc = g2s_fill_sets(s, gv.data(), gs.data(), gv.size(), res.data(), arena.data(), arena.size());
    if (rc != G2S_OK) {
      std::cerr << "Gap2Seq-libraries: " << g2s_last_error() << std::endl;
      g2s_session_destroy(s);
      g2s_graph_free(graph);
      return EXIT_FAILURE;
    }
    for (size_t q = 0; q < gv.size(); q++) {  // the sequence of g2s_execute_single's FASTA (Gap2Seq.cpp:266-273)
      const GapRec& g = gaps[idx[q]];
      const g2s_result& r = res[q];
      if (r.count > 0 && (!unique || r.count == 1))
        fills[idx[q]] = g.left.substr(0, g.left.size() - (size_t)r.left_fuz) + std::string(arena.data() + r.fill_off);
    }
    g2s_session_destroy(s);
    g2s_graph_free(graph);
    lo = hi;
  }
  // ---- output in input order; a gap without a fill: left + N * gap + right (Gap2Seq.py:210)
  std::string out;
  size_t successful = 0;
  for (size_t i = 0; i < ngaps; i++) {
    const GapRec& g = gaps[i];
    if (fills[i].empty()) fills[i] = g.left + std::string((size_t)std::max(0, g.gap_length), 'N') + g.right;
    if (fills[i].find_first_of("Nn") == std::string::npos) successful++;  // (Gap2Seq.py:216)
    out += g.comment + "\n" + fills[i] + "\n";
  }
  FILE* f = fopen(filled_path.c_str(), "wb");
  if (!f) { std::cerr << "Gap2Seq-libraries: cannot write " << filled_path << std::endl; return EXIT_FAILURE; }
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  for (g2s_read_pool* P : host_pools) g2s_read_pool_free(P);
  for (g2s_device_pool* P : dev_pools) g2s_device_pool_free(P);
  std::cout << "Filled " << successful << " out of " << ngaps << " gaps" << std::endl;  // (Gap2Seq.py:513)
  return EXIT_SUCCESS;
}
