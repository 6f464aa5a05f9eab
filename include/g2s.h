/* ===========================================================================
 *  include/g2s.h — C ABI of the MI355X-native Gap2Seq-core fill path.
 *
 *  This is the drop-in boundary.  The reference has no FFI of its own: the hot
 *  path is the in-process C++ member
 *      int Gap2Seq::fill_gap(const Graph&, const std::string& kmer_left,
 *                            const std::string& kmer_right, int gap_len, int k,
 *                            int gap_err, int left_max_fuz, int right_max_fuz,
 *                            int* left_fuz, int* right_fuz, long long max_mem,
 *                            char* fill, bool skip_confident, bool all_paths,
 *                            subgraph_stats*)
 *  (/root/reference/src/Gap2Seq.hpp:74-76, Gap2Seq.cpp:858-1556), called once
 *  per gap from Gap2Seq::execute() (Gap2Seq.cpp:252 and :380) on a GATB Graph
 *  built once (Gap2Seq.cpp:193-219).  Each entry point below names the piece of
 *  that interface it replaces.  INTEGRATION.md shows the stub a maintainer of
 *  the reference would add to call it.
 *
 *  Plain C: opaque handles, caller-owned buffers, integer status codes, no
 *  exceptions cross this boundary.  One g2s_session drives one GPU; sessions
 *  on different devices may run on different host threads.
 *  There is NO CPU fallback: every fill entry point returns G2S_ERR_NO_DEVICE
 *  when no gfx950 device is usable.
 * ======================================================================== */
#ifndef G2S_H_
#define G2S_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G2S_ABI_VERSION 6

/* status codes */
#define G2S_OK 0
#define G2S_ERR_ARG (-1)
#define G2S_ERR_IO (-2)
#define G2S_ERR_NO_DEVICE (-3)
#define G2S_ERR_HIP (-4)
#define G2S_ERR_NOMEM (-5)
#define G2S_ERR_STATE (-6)

/* Gap2Seq.cpp:38 */
#define G2S_MAX_PATHS (2147483647 / 2 - 1)
#define G2S_INVALID_NODE 0xFFFFFFFFu

typedef struct g2s_graph g2s_graph;     /* replaces gatb Graph (host + device copies) */
typedef struct g2s_session g2s_session; /* one device, one rand() stream, reusable workspaces */
typedef struct g2s_batch g2s_batch;     /* a prepared list of gaps resident in HBM */

int g2s_abi_version(void);
/* Thread-local text of the last error returned on this thread. */
const char* g2s_last_error(void);

/* ---------------------------------------------------------------------------
 *  Graph: replaces Graph::create(BankAlbum, "-kmer-size k -abundance-min solid
 *  ...") / Graph::load (Gap2Seq.cpp:193-219).  Exact solid canonical k-mer set
 *  (GATB codec A0 C1 T2 G3, canonical = min(fwd, revcomp), k-mers containing
 *  N/n skipped; k in [1, 127]: 64-, 128- or 256-bit k-mers), numbered in unitig order, with a 4-slot successor table per
 *  oriented node in GATB enumeration order (A,C,T,G).  At odd k predecessors are
 *  read from the same table: pred(v)[i] = succ(v^1)[i]^1.  At even k a k-mer
 *  can be its own reverse complement; only one strand of such a k-mer exists,
 *  the identity fails next to it, and the graph carries an explicit
 *  predecessor table (g2s_graph_predecessors reads whichever applies).  Such a
 *  graph fills on the same kernels as any other (segment tier, resident mode):
 *  a session derives the table of their backward walks from the predecessor table.
 *  The build itself (k-mer sort, successor table, unitig numbering) runs on
 *  the GPU named by the environment variable G2S_DEVICE (default 0) when there
 *  is one, and the graph then already resides on that device; without a
 *  device or with G2S_HOST_BUILD=1 it runs on `nthreads` host
 *  threads.  Either way the same graph results, up to the numbering of nodes.
 *  Read sets beyond one device sort (2^32 positions — bases + 1 a read — or half
 *  the free device memory at 56-104 bytes a position) stay on the device: the
 *  reads are kept there as text and the solid k-mers are counted in key-range
 *  passes.  The host counts them only when the text does not fit beside one
 *  pass or one k-mer alone occurs more often than a pass holds keys
 *  (G2S_DEBUG=1 says which).  The graph itself holds fewer than 2^30 k-mers
 *  (g2s_graph_build_seqs_reach / _files_reach below: a graph bounded to a gap list's reach, the cap on what is kept).
 *  g2s_graph_build_files: reads_csv is a comma-separated list of FASTA/FASTQ
 *  files; gzip-compressed ones (plain gzip or BGZF, recognised by their magic
 *  bytes, not their names) are read transparently.  BAM files may stand in
 *  the list too, in any order: a file is BAM when it is gzip, its first
 *  member is a BGZF member and its inflated stream begins with "BAM\1".
 *  Every alignment record that is neither secondary (0x100) nor
 *  supplementary (0x800) gives one sequence, mapped or not, in file order —
 *  the reads `samtools fastq` would emit: the 4-bit codes 1, 2, 4, 8 are
 *  A, C, G, T, every other code is N, and a reverse-strand record (0x10) is
 *  reverse-complemented back to the read as sequenced; a record without
 *  bases is an empty sequence.  With a usable device the
 *  files' bytes are parsed there and never form sequences on the host
 *  (G2S_HOST_READS=1: the host loader).  A BAM file is held on the device
 *  whole — inflated stream, rows and text — while that fits half the free
 *  device memory; a larger one goes through two windows of the inflate, its
 *  text written window by window, and is bounded by its text alone: a
 *  buffer of two thirds of its inflated size and a fixed amount beside it
 *  (G2S_BUILD_BAM_STREAM=1|0: that form always, never).  G2S_ERR_IO with the file's name in
 *  g2s_last_error() for a file that cannot be read or whose gzip stream is
 *  truncated or corrupt, and for a BAM file with a member that does not
 *  inflate, a cut record or a header that does not parse.
 * ------------------------------------------------------------------------ */
int g2s_graph_build_files(const char* reads_csv, int k, int solid, int nthreads, g2s_graph** out);
int g2s_graph_build_seqs(const char* const* seqs, const uint64_t* lens, int nseqs, int k, int solid,
                         int nthreads, g2s_graph** out);
/* Set graphs: one graph per read set in one handle, for the wrapper's per-gap libraries flow (Gap2Seq.py:133-218:
 * a fresh Gap2Seq-core over each gap's own reads).  seqs[j] belongs to set seq_set[j] < nsets; every set's graph is
 * built from its own sequences alone (solidity counted per set) with the same k and solid.  Node indices are
 * numbered set-major: set s holds one contiguous range [first_kmer, first_kmer + n_kmers) of node indices (oriented
 * ids 2*index + strand), the sets' ranges follow in set order, and no edge leaves a set.  A set may be empty.
 * nsets == 1 gives an ordinary graph (what g2s_graph_build_seqs gives); otherwise g2s_graph_node returns
 * G2S_INVALID_NODE (a k-mer is a different node in every set it is solid in): use g2s_graph_set_node.  Graphs of
 * several sets are built on host threads and cannot be saved (g2s_graph_save: G2S_ERR_ARG). */
int g2s_graph_build_sets(const char* const* seqs, const uint64_t* lens, const uint32_t* seq_set, int nseqs, uint32_t nsets,
                         int k, int solid, int nthreads, g2s_graph** out);
/* The same set graph from a POOL of sequences that the sets share (ABI 6, additive), for read sets that overlap — the
 * libraries flow's gaps select the same reads again and again, and every gap under the threshold takes every unmapped
 * read.  Set s is the MULTISET of the sequences seqs[set_seq[q]], q in [set_begin[s], set_begin[s+1]) (its own list),
 * followed by seqs[shared_seq[0 .. nshared)] when set_shared[s] is nonzero.  The graph is the one
 * g2s_graph_build_sets gives for that expanded list: the same sets, the same solid k-mers per set, the same edges,
 * set-major numbering, g2s_graph_set_nodes equal (the numbering of nodes inside a set may differ where the host and
 * the device build differ).  A sequence may be in any number of sets and more than once in one set; every occurrence
 * counts towards solidity, as the concatenated FASTA files count it in the reference flow.  No text is copied on the
 * host.  On the device (any k) the pool's text goes up once, the own lists' k-mers are sorted by (set, k-mer), and the
 * shared list's k-mers are sorted ONCE and merged into every flagged set, so the keys sorted are the own lists'
 * positions plus the shared list's, whatever the number of flagged sets; when the device cannot take it (the own and
 * shared positions reach 2^32, the estimate exceeds half the free device memory — the merge's flagged sets x distinct
 * shared k-mers included — or 2^30 k-mers result) the host builds it set by set from each set's pointers, as for even
 * k, without a device and with G2S_HOST_BUILD=1 (G2S_DEBUG=1 says which, and why).
 * shared_seq may be NULL when nshared == 0; set_shared NULL = no set holds the shared list; nsets == 1 gives an
 * ordinary graph.  G2S_ERR_ARG: an index >= nseqs, nseqs >= 2^32, a decreasing set_begin, nsets == 0, k out of range;
 * *out is not written then. */
int g2s_graph_build_pool(const char* const* seqs, const uint64_t* lens, uint64_t nseqs,
                         const uint64_t* set_begin,   /* [nsets + 1] */
                         const uint32_t* set_seq,     /* [set_begin[nsets]] indices into seqs */
                         const uint32_t* shared_seq,  /* [nshared] indices into seqs */
                         uint64_t nshared,
                         const uint8_t* set_shared,   /* [nsets] */
                         uint32_t nsets, int k, int solid, int nthreads, g2s_graph** out);
struct g2s_gap;
/* g2s_graph_build_pool with every set bounded to the k-mers its gap's fill can reach (ABI 6, additive).  The first
 * thirteen arguments are g2s_graph_build_pool's.  Set s with reach_radius[s] >= 0 has a REACH RECORD, the gap
 * reach_gap[s], and is built as follows:
 *   full graph  what g2s_graph_build_pool builds for s: the solid canonical k-mers of its own list (+ the shared list
 *               when flagged);
 *   seeds       the flank k-mers the fill looks up for reach_gap[s] (the (lmf+1) k-mers of left[0 .. k+lmf), the
 *               (rmf+1) k-mers of the last k+rmf characters of right and the (rmf+1) of its first k+rmf), encoded as
 *               the fill encodes them; none for a gap the fill rejects (NULL flank, negative lmf / rmf / gap_len,
 *               left_len < k+lmf or right_len < k+rmf).  A seed that is no k-mer of the full graph is ignored;
 *   kept set    every k-mer of the full graph at an undirected distance <= reach_radius[s] of some seed, the distance
 *               counted over canonical k-mers, each with its eight possible neighbours (four extensions either way);
 *   the set     the subgraph of the full graph induced on the kept set; EMPTY when no seed is in the full graph.
 * reach_radius[s] < 0: the whole set, as g2s_graph_build_pool builds it (reach_gap[s] is not read).  Numbering is
 * set-major and g2s_graph_set_nodes works as for any set graph.  With both arrays NULL, or every radius negative, the
 * graph is g2s_graph_build_pool's.
 *   SOUND RADIUS: for a fill with g2s_params.d_err = d_err the radius max(0, gap_len + d_err) + lmf + rmf loses
 * nothing — the search of fill_gap is depth-bounded (right search: right_half; left search: left_half + right_half
 * = gap_len + d_err + lmf + rmf, Gap2Seq.cpp:862-863, 908, 1029), so g2s_fill_sets gives the same results on the
 * bounded graph as on the whole one.  The bound is safe, not tight: the kept set is the union of the balls round ALL
 * seeds, the right flank's included, so a closing path of L steps is kept whole from radius (L - 1) / 2 on and a fill
 * first changes one below that (tests/test_gpu_pool_reach.py pins both sides).
 *   On the device (any k) the bounded sets are found by a breadth-first search per set over the own lists' and the
 * shared list's sorted count tables — membership of a k-mer is two binary searches, the sets' full graphs are never
 * formed, and the work and the memory follow the k-mers visited plus one bit a (set with a record, distinct shared
 * k-mer) instead of flagged sets x distinct shared k-mers.  When the device cannot take it (the conditions of
 * g2s_graph_build_pool — its flagged sets x shared k-mers term counting the flagged sets WITHOUT a record only — the
 * kept k-mers exceeding the search's queue at its largest — it starts at the own k-mers plus 4 096 a set and grows on
 * overflow, never sized by sets x shared k-mers up front — or a level of one set exceeding its chunk list) the host builds the
 * same graph by a search per set, also without forming a full graph (G2S_DEBUG=1 says which, and why).
 * G2S_ERR_ARG: g2s_graph_build_pool's, and exactly one of the two arrays NULL; *out is not written then. */
int g2s_graph_build_pool_reach(const char* const* seqs, const uint64_t* lens, uint64_t nseqs,
                               const uint64_t* set_begin, const uint32_t* set_seq, const uint32_t* shared_seq,
                               uint64_t nshared, const uint8_t* set_shared, uint32_t nsets, int k, int solid, int nthreads,
                               const struct g2s_gap* reach_gap,  /* [nsets], or NULL */
                               const int32_t* reach_radius,      /* [nsets], or NULL */
                               g2s_graph** out);
/* ---------------------------------------------------------------------------
 *  A SINGLE graph bounded to what a gap list can reach (ABI 6, additive): g2s_graph_build_seqs / _files plus reach
 *  records, for read sets whose solid k-mers number 2^30 and more — the cap of 32-bit oriented node ids then applies to
 *  what the gaps can touch, not to the read set.  reach_gap[r] with reach_radius[r] >= 0, r < nreach, is a record:
 *    full set    the solid canonical k-mers the plain call would find;
 *    seeds of r  the seeds g2s_graph_build_pool_reach defines for reach_gap[r] (none for a gap the fill rejects); a seed
 *                outside the full set is ignored;
 *    kept set    every k-mer of the full set at an undirected distance <= reach_radius[r] of a seed of SOME record r, the
 *                distance counted over canonical k-mers with their eight neighbours, as for the pool form;
 *    the graph   what the plain call gives for the kept set: the induced subgraph, one set, ordinary numbering; EMPTY
 *                with nreach == 0 or no seed in the full set.
 *  At the SOUND RADIUS (above) of every gap of a list the fills on the bounded graph equal those on the whole one.
 *  mode: G2S_REACH_ALWAYS the bounded graph; G2S_REACH_NEVER the plain call; G2S_REACH_AUTO the plain call, bit for bit —
 *  and only when that fails with "too many k-mers for 32-bit oriented node ids" the build starts over bounded, so only
 *  inputs that fail today pay for it (G2S_BUILD_REACH=1|0 in the environment turns AUTO into ALWAYS | NEVER).
 *  Both arrays NULL: the plain call whatever the mode.  The cap (2^30 k-mers; G2S_BUILD_MAX_KMERS=N lowers it, for
 *  tests) applies to the KEPT set.  On the device the full set stays in device memory as one sorted table of any size
 *  that fits beside the text and one pass — the one sort's result, or the key-range passes' results one behind the other —
 *  and one level-synchronous search over the whole chip serves all records (csrc/graph_reach.h); an allocation that
 *  fails or a HIP error hands the build to the host path (G2S_DEBUG=1 says why), where the bound is host memory and the
 *  same search runs on `nthreads` threads.  Either way the same graph, node for node.
 *  G2S_ERR_ARG: a negative radius, exactly one of the arrays NULL with nreach > 0, an unknown mode, and the plain call's;
 *  *out is not written then. */
#define G2S_REACH_NEVER 0
#define G2S_REACH_ALWAYS 1
#define G2S_REACH_AUTO 2
int g2s_graph_build_seqs_reach(const char* const* seqs, const uint64_t* lens, int nseqs, int k, int solid, int nthreads,
                               const struct g2s_gap* reach_gap, const int32_t* reach_radius, uint64_t nreach, int mode,
                               g2s_graph** out);
int g2s_graph_build_files_reach(const char* reads_csv, int k, int solid, int nthreads, const struct g2s_gap* reach_gap,
                                const int32_t* reach_radius, uint64_t nreach, int mode, g2s_graph** out);
/* The reach records of a scaffolds file for g2s_execute_scaffolds with max_fuz and g2s_params.d_err = d_err: one record
 * per N-run [istart, iend) of every scaffold record, in input order.
 *   left flank   seq[a, istart) with a = max(the previous run's end, istart - k - max_fuz, 0), lmf = its length - k (a
 *                window shorter than k gives a record without seeds: the scanner cannot fill that gap either);
 *   right flank  seq[iend, iend + k + rmf), rmf as the scanner takes it; where the scanner finds no usable right flank
 *                the record has no seeds;
 *   radius       max(0, gap + d_err) + lmf + rmf.
 * Whatever the previous gap's right_fuz was, the left flank the scanner hands the fill lies inside that window and its
 * left_max_fuz is at most lmf, so every record holds a superset of the fill's seeds at a radius at least the fill's own.
 * The handle owns the flank strings; the arrays hold g2s_reach_records_count() entries and live until
 * g2s_reach_records_free. */
typedef struct g2s_reach_records g2s_reach_records;
int g2s_scaffolds_reach(const char* scaffolds_text, int k, int max_fuz, int d_err, g2s_reach_records** out);
uint64_t g2s_reach_records_count(const g2s_reach_records* r);
const struct g2s_gap* g2s_reach_records_gaps(const g2s_reach_records* r);
const int32_t* g2s_reach_records_radii(const g2s_reach_records* r);
void g2s_reach_records_free(g2s_reach_records* r);
/* 1 for a graph that reach records bounded (g2s_graph_build_seqs_reach / _files_reach on the bounded path): it belongs to
 * its gap list, and a caller that caches graphs by their reads (Gap2Seq-core's "<reads>.g2s") must not cache it. */
int g2s_graph_bounded(const g2s_graph* g);
uint32_t g2s_graph_num_sets(const g2s_graph* g); /* 1 for every graph built the other ways */
int g2s_graph_set_nodes(const g2s_graph* g, uint32_t set, uint64_t* first_kmer, uint64_t* n_kmers);
uint32_t g2s_graph_set_node(const g2s_graph* g, uint32_t set, const char* kmer); /* G2S_INVALID_NODE if absent */
/* Own binary cache (the reference reuses "<reads>.h5", Gap2Seq.cpp:171,195-197). */
int g2s_graph_save(const g2s_graph* g, const char* path);
int g2s_graph_load(const char* path, g2s_graph** out);
void g2s_graph_free(g2s_graph* g);
int g2s_graph_k(const g2s_graph* g);
/* -solid the set was built with (0: a cache file written before this was recorded). */
int g2s_graph_solid(const g2s_graph* g);
uint64_t g2s_graph_num_kmers(const g2s_graph* g);
uint64_t g2s_graph_num_unitigs(const g2s_graph* g);
/* graph.buildNode + graph.contains: oriented node id (2*index + strand) of the
 * first k characters of `kmer`, or G2S_INVALID_NODE when it is not solid. */
uint32_t g2s_graph_node(const g2s_graph* g, const char* kmer);
/* graph.successors / graph.predecessors in GATB order; returns the count. */
int g2s_graph_successors(const g2s_graph* g, uint32_t node, uint32_t out[4]);
int g2s_graph_predecessors(const g2s_graph* g, uint32_t node, uint32_t out[4]);
/* graph.toString(node): writes k chars + NUL. */
int g2s_graph_node_string(const g2s_graph* g, uint32_t node, char* out);
/* Copy the successor table into the HBM of `device` (idempotent per device). */
int g2s_graph_upload(g2s_graph* g, int device);
/* Bytes resident in HBM for this graph on `device` (0 when not uploaded). */
uint64_t g2s_graph_device_bytes(const g2s_graph* g, int device);

/* ---------------------------------------------------------------------------
 *  Parameters: the Gap2Seq-core options that reach fill_gap
 *  (Gap2Seq.cpp:164-175).
 * ------------------------------------------------------------------------ */
typedef struct g2s_params {
  int32_t d_err;          /* -dist-error (gap_err)                       */
  int32_t skip_confident; /* -all-upper                                  */
  int32_t all_paths;      /* !-best-only                                 */
  int32_t unique_paths;   /* -unique (applied by the caller of fill_gap) */
  int64_t max_mem;        /* bytes per gap, already divided by threads
                             (Gap2Seq.cpp:170,302); device-budget analogue */
  uint32_t randseed;      /* -randseed: srand() argument; 0 = time(NULL) (Gap2Seq.cpp:178) */
  int32_t host_threads;   /* threads for the per-gap host post-process; 0 = all */
} g2s_params;

/* One fill_gap call's inputs (Gap2Seq.cpp:380-383 / :252-254). */
typedef struct g2s_gap {
  const char* left;   /* kmer_left : k+lmf chars (longer allowed, as in -left)  */
  const char* right;  /* kmer_right: k+rmf chars                                */
  int32_t left_len;
  int32_t right_len;
  int32_t gap_len;
  int32_t lmf;        /* left_max_fuz  */
  int32_t rmf;        /* right_max_fuz */
  /* Scaffold scanning continues at i += right_fuz after a filled gap
   * (Gap2Seq.cpp:402,415), which can make the NEXT gap of the same record
   * ineligible.  If >= 0: skip this gap (status G2S_GAP_SKIPPED, no rand()
   * draws) when the previous gap of the batch was filled with right_fuz
   * greater than this value.  -1: independent. */
  int32_t skip_if_prev_right_fuz_gt;
} g2s_gap;

/* g2s_result.flags */
#define G2S_GAP_SKIPPED 0x1        /* see skip_if_prev_right_fuz_gt                     */
#define G2S_GAP_Q7 0x2             /* both strands of one k-mer met: result is
                                      well defined but outside the bit-exact claim        */
#define G2S_GAP_MEM_EXCEEDED 0x4   /* count == -1                                         */
#define G2S_GAP_BACKTRACE_FAIL 0x8 /* "Unable to backtrace!" (Gap2Seq.cpp:1493-1510)      */
#define G2S_GAP_BAD_FLANK 0x10     /* flank shorter than k+fuz (reference would throw)    */
#define G2S_GAP_PHASE_D 0x20       /* phase D ran: fill / left_fuz / right_fuz written    */

typedef struct g2s_result {
  int32_t count;      /* fill_gap return value: >0 paths (saturating), 0, or -1 */
  int32_t left_fuz;
  int32_t right_fuz;
  uint32_t flags;
  /* `fill` as the reference leaves it: the useful text starts at
   * buf[lmf - left_fuz]; here fill_off points at exactly that position inside
   * the caller's arena and fill_len = strlen(&buf[lmf-left_fuz]) (it INCLUDES
   * the right k-mer, Gap2Seq.cpp:856-857).  NUL terminated. */
  uint64_t fill_off;
  int32_t fill_len;
  int32_t draws;      /* rand() calls consumed */
  /* subgraph_stats (Gap2Seq.hpp:50-58); valid when count > 0 and !skip_confident */
  uint64_t vertices, edges, nontrivial_components, size_nontrivial_components, vertices_final, edges_final;
  /* phase C result before the D1 recount */
  int32_t phaseC_count;
  int32_t n_lengths;
  int32_t lengths[2];
  /* G2S_GAP_BACKTRACE_FAIL: the two numbers of the reference's "Unable to backtrace!" line (Gap2Seq.cpp:1494:
   * currentD2, currentD); g2s_backtrace_text() makes the line.  (ABI 3 carried the 96-byte text in every record:
   * 1.9 MB of a 10 000-gap list's 7.7 MB over the link, for a line no gap of the test lists ever printed.) */
  int32_t backtrace_depth, backtrace_final_d;
  int32_t reserved[2];    /* the record is 112 bytes: seven 16-byte stores of the trace kernel */
} g2s_result;

/* Lists in flight on one GPU, for a caller that streams lists (Gap2Seq-core -stream-gaps; the reference prints a gap
 * when it is done and goes on, Gap2Seq.cpp:385,426-431).  g2s_fill_begin() takes a list as g2s_fill_batch() does,
 * queues its kernels and returns; g2s_fill_end() finishes the OLDEST list begun (results and fill text in that list's
 * buffers, which must stay valid until then) and returns what g2s_fill_batch() would.  At most G2S_MAX_IN_FLIGHT lists
 * may be begun and not ended: the younger ones' kernels then run while the oldest one's results cross the link and the
 * host prepares the next.  Lists end in the order they were begun and draw from the session's one rand() stream in
 * that order: results are identical to g2s_fill_batch() list by list.  g2s_fill_in_flight(): lists begun, not ended.
 * While lists are in flight the session's buffers and its rand() stream belong to them: g2s_fill_batch,
 * g2s_batch_prepare, g2s_batch_run, g2s_team_fill (with this session in the team), g2s_session_set_team,
 * g2s_session_srand and g2s_session_skip_draws return G2S_ERR_STATE and do nothing until every list has been ended
 * (ABI 5; g2s_session_destroy may be called at any time: it waits for the lists' kernels and drops them).
 *
 * A session with a team (g2s_session_set_team, G2S_GROUP_PER_SESSION): a list long enough for one share per session,
 * in g2s_host_alloc buffers, no record cut by a share boundary, has the first step of every share — preparation,
 * look-ups, fill kernel, classes and totals — queued on that share's device by g2s_fill_begin(), on the member's
 * session or on a twin of it on the same device (three lists in flight: three sets of streams and buffers per GPU).
 * That step reads nothing of the rand() stream.  g2s_fill_end() waits for the shares' totals, places the shares in the
 * stream from where the lead's generator then stands, and runs the tables and the tracebacks on the same sessions:
 * they overlap the first step of the lists begun behind.  A list that then turns out not to be one for the devices is
 * run by g2s_fill_end() as g2s_fill_batch() would run it; the lists behind it keep what they queued.  Any other list of
 * a team (pageable buffers, a record across a share boundary, G2S_TEAM_IN_FLIGHT=0) waits for g2s_fill_end() with all
 * of its work, on the team's own sessions, which nothing begun behind it uses.  While the lead has lists in flight its
 * helpers refuse what the lead refuses (their buffers carry shares); the lead is to be destroyed before its helpers, or
 * its lists ended first — a helper destroyed under its lead's lists waits for their kernels and drops them all.
 * g2s_fill_in_flight_launched(): how many of the lists in flight have their fill kernels queued on the device(s). */
#define G2S_MAX_IN_FLIGHT 3
int g2s_fill_begin(g2s_session* s, const g2s_gap* gaps, size_t n, g2s_result* results, char* fill_arena, size_t arena_cap);
int g2s_fill_end(g2s_session* s);
int g2s_fill_in_flight(const g2s_session* s);
int g2s_fill_in_flight_launched(const g2s_session* s);

/* The reference's line for a gap flagged G2S_GAP_BACKTRACE_FAIL (Gap2Seq.cpp:1494): "Unable to backtrace! <currentD2>
 * <currentD> <toString(reachedTarget)>", without the newline; the k-mer is right[right_fuz .. right_fuz + k) in upper
 * case (the node was built from that text, Gap2Seq.cpp:1113).  Returns the length, or 0 when the gap is not flagged. */
size_t g2s_backtrace_text(const g2s_gap* gap, const g2s_result* r, int k, char* out, size_t cap);

/* Per-batch measurements (bench.py). */
typedef struct g2s_timing {
  double ms_right_bfs;    /* kernel g2s_right_bfs (HBM tier), HIP events on the session stream */
  double ms_left_dp;      /* kernel g2s_left_dp  (HBM tier frontier kernel)         */
  double ms_extract;      /* kernel g2s_extract  (HBM tier)                         */
  double ms_d2h;
  double ms_host_post;    /* SCC / branch rule / traceback on the host              */
  double ms_total;        /* wall time of g2s_batch_run                             */
  uint64_t xA, sA, xB, sB, xD, sD; /* expansions / newly set states per phase, counted on device */
  uint64_t flank_bytes;   /* sum over gaps of (k+lmf)+(k+rmf)                       */
  uint64_t fill_bytes;    /* sum over gaps of fill_len                              */
  uint32_t launches_left_dp; /* >1 when overflowing gaps were retried with larger tables */
  uint32_t retried_gaps;
  /* retired tier (round 1's level-by-level kernels in LDS), kept for the layout: always zero */
  double ms_fill_lds;
  double ms_extract_lds;
  uint64_t x_fill_lds;
  uint64_t s_fill_lds;
  uint32_t lds_tier_gaps;
  uint32_t lds_launches;
  uint32_t log_pool_gaps;
  uint32_t rs_pool_gaps;
  double ms_prepare;         /* g2s_fill_batch / g2s_team_fill: flank k-mer -> node resolution + descriptor upload
                                (g2s_batch_prepare), inside ms_total; summed over sessions for a team */
  /* segment tier (kernel g2s_fill_seg = phases A-D1 over unitig segments, fill_seg.hip) */
  double ms_fill_seg;        /* HIP events on the session stream, summed over the launches that were bracketed with
                                events: all on the host path, one in eight in resident mode (seg_timed_launches;
                                G2S_KERNEL_TIMING=all times every launch) */
  uint32_t seg_tier_gaps;    /* gaps that completed in the segment tier */
  uint32_t seg_launches;
  uint64_t seg_segments;     /* segments those gaps took (a config-2 gap: ~25 for ~1000 DP states) */
  double ms_fill_segx;       /* the tier's large variant (g2s_fill_segw): gaps that outgrow the LDS-resident capacities */
  uint32_t segx_tier_gaps;
  uint32_t segx_launches;
  uint32_t watchdog_gaps;    /* gaps on which a probe loop of the large variant ran past its bound (a defect; expected 0) */
  uint32_t seg2_launches;    /* segment-tier launches that ran two waves per gap (g2s_fill_seg2: short lists) */
  /* resident mode: the whole list on the device, phase D3 included (d3_device.hip) */
  double ms_d3;              /* kernels of phase D3 behind the fill kernel (scan, rand() stream, tables, chain, tracebacks) */
  uint32_t resident_launches;   /* lists (groups) finished on the device */
  uint32_t resident_fallbacks;  /* lists the device gave back to the host path */
  uint64_t draw_dependent_gaps; /* gaps whose number of rand() draws depends on the values drawn */
  uint64_t d3_table_entries;    /* entries of the draw-count tables that resolved their offsets */
  uint32_t host_finished_gaps;  /* gaps of resident lists whose closure the host analysed and traced (a k-mer at two depths) */
  /* g2s_team_fill: the dispatcher's groups and which session took how many (sessions beyond the 16th are not listed) */
  uint32_t team_groups, team_sessions;
  uint32_t team_groups_by_session[16];
  uint32_t seg_timed_launches;  /* segment-tier launches whose duration is in ms_fill_seg (and, resident mode, in ms_d3) */
  uint32_t team_d3_sharded;     /* g2s_team_fill: every session traced its own group and wrote its own results (phase D3 sharded) */
  uint32_t traced_in_fill_gaps; /* (ABI 6) gaps of resident lists whose fill kernel's wave wrote fill text and record itself: a traceback
                                   with one path length and no choice between parents writes the same whatever rand() returns */
  /* ...and, per session (the first 16), what its group took: fill kernel(s) and phase D3 kernels by HIP events (timed
   * launches only), and the wall time of the session's thread from the call to its last result */
  double team_ms_fill[16], team_ms_d3[16], team_ms_wall[16];
  /* (ABI 6) g2s_fill_batch on one session, resident mode: where the host's time inside the call goes, in microseconds:
   * [0] entry -> fill kernel queued (preparation and launch set-up: the device idles until then), [1] -> phase D3
   * queued, [2] -> the device's hand-over seen (waiting), [3] -> the host-finished gaps done, [4] -> stream
   * synchronised, [5] -> return.  Zero when the list took another path. */
  double host_us[8];
  /* (ABI 6) ... and whose fill kernel's wave wrote a GUESS of a traceback that has choices (first path length, first
   * parent at every choice); of those gaps' text, in groups of 64 bases as the trace kernel's first waves compared them:
   * all / sent through the link again because the real traceback differs there */
  uint32_t guessed_in_fill_gaps, guessed_groups, guessed_groups_resent, reserved1;
} g2s_timing;

/* ---------------------------------------------------------------------------
 *  Session: owns the device, the stream, the reusable workspaces and the
 *  glibc-compatible rand() stream that the traceback consumes in gap order.
 * ------------------------------------------------------------------------ */
int g2s_session_create(g2s_graph* g, int device, const g2s_params* p, g2s_session** out);
void g2s_session_destroy(g2s_session* s);
/* srand(seed) (Gap2Seq.cpp:178).  G2S_OK, or G2S_ERR_STATE with lists in flight (ABI 5: void before). */
int g2s_session_srand(g2s_session* s, uint32_t seed);
/* Discard the next n values of the session's rand() stream: what n calls of rand() by the
 * caller between two fill_gap calls would do to the reference's libc stream.  Returns as g2s_session_srand. */
int g2s_session_skip_draws(g2s_session* s, uint64_t n);

/* Resolve flank k-mers to node ids on the host and upload the gap descriptors
 * to HBM.  Replaces the argument marshalling of Gap2Seq.cpp:380-383. */
int g2s_batch_prepare(g2s_session* s, const g2s_gap* gaps, size_t n, g2s_batch** out);
/* The hot path: phases A-D of fill_gap for every gap of the batch (kernels on
 * the session stream, device->host of the state logs, host SCC/branch rule and
 * the in-order traceback).  `fill_arena` receives the NUL-terminated fills;
 * it needs sum(gap_len + k + d_err + lmf + rmf + 3) bytes (g2s_batch_arena_bytes). */
int g2s_batch_run(g2s_batch* b, g2s_result* results, char* fill_arena, size_t arena_cap);
size_t g2s_batch_arena_bytes(const g2s_batch* b);
int g2s_batch_timing(const g2s_batch* b, g2s_timing* out);
void g2s_batch_free(g2s_batch* b);
/* Measurements of the last g2s_fill_batch / g2s_batch_run on this session (ms_total = wall
 * time of that call, preparation included for g2s_fill_batch). */
int g2s_session_last_timing(const g2s_session* s, g2s_timing* out);
/* prepare + run + free. */
int g2s_fill_batch(g2s_session* s, const g2s_gap* gaps, size_t n, g2s_result* results, char* fill_arena,
                   size_t arena_cap);
/* Independent gaps over a set graph (g2s_graph_build_sets): gap i is filled in set gap_set[i] alone, with a rand()
 * stream that starts from srand(randseed) for every gap, as a fresh Gap2Seq-core -reads S(i) -left L -right R
 * -length G -randseed randseed would (g2s_execute_single on a one-set graph of S(i), Gap2Seq.cpp:227-283).  A gap's
 * result depends neither on its position in the list nor on the other gaps, and the session's own stream is not
 * advanced.  Several gaps may name one set.  randseed 0 takes the seed the session was created with.
 * Arena as for g2s_fill_batch.  G2S_ERR_ARG: a set id out of range, a gap with skip_if_prev_right_fuz_gt != -1;
 * G2S_ERR_STATE: lists in flight, or the session is in a team.  Groups of 256 gaps or more are finished on the device
 * like any list (resident mode, G2S_RESIDENT=0|1 as for g2s_fill_batch): phase D3 in its restart form — every gap reads
 * the stream from value 0, nothing is consumed; a group the device gives back takes the host path.  The timing of the
 * call (g2s_session_last_timing) sums the groups', the resident counters included. */
int g2s_fill_sets(g2s_session* s, const g2s_gap* gaps, const uint32_t* gap_set, size_t n, g2s_result* results,
                  char* fill_arena, size_t arena_cap);

/* ---------------------------------------------------------------------------
 *  Several sessions on one gap list = the reference's dispatcher
 *  (`-nb-cores`, Gap2Seq.cpp:300-304: threads pulling scaffolds from a shared
 *  iterator), with GPUs in place of threads.  The list is cut into groups of
 *  `group_size` gaps (0 = default); each session's host thread pulls the next
 *  group from a shared counter and runs phases A-D2 for it; the rand()
 *  dependent part (D3) then runs once, in gap order, on sessions[0]'s stream,
 *  so results equal g2s_fill_batch(sessions[0], ...) bit for bit.  Sessions
 *  must share one graph; they may sit on different devices (graph replicated,
 *  no exchange step) or on the same device (one session's host analysis then
 *  overlaps the other's kernels).  `timing` (optional) receives the sums over
 *  groups with ms_total = wall time of the call.
 *  g2s_session_set_team makes g2s_fill_batch / g2s_execute_* on `lead` use
 *  lead + helpers this way for lists longer than group_size; helpers must
 *  outlive the lead or be detached with nhelpers = 0.
 * ------------------------------------------------------------------------ */
int g2s_team_fill(g2s_session* const* sessions, int nsessions, const g2s_gap* gaps, size_t n, size_t group_size,
                  g2s_result* results, char* fill_arena, size_t arena_cap, g2s_timing* timing);
size_t g2s_team_arena_bytes(const g2s_session* s, const g2s_gap* gaps, size_t n);
int g2s_session_set_team(g2s_session* lead, g2s_session* const* helpers, int nhelpers, size_t group_size);
/* group_size for g2s_session_set_team: every list of at least 512 gaps per session is cut into ONE group per session
 * (a whole share of the list per GPU: each GPU fills, traces and writes its own share, the rand() stream chained from
 * share to share by draw totals — what a caller that streams long lists over several GPUs wants; Gap2Seq-core -devices) */
#define G2S_GROUP_PER_SESSION ((size_t)-1)

/* ---------------------------------------------------------------------------
 *  One list over several PROCESSES, one GPU each (ABI 6) — for a launcher that pins a device per rank (torchrun with
 *  HIP_VISIBLE_DEVICES per rank), where g2s_team_fill's one process cannot see the other GPUs.  The reference's threads
 *  share one rand() stream (Gap2Seq.cpp:178,296-306, at -nb-cores 1: in input order); here every rank fills,
 *  classifies, traces and writes ITS contiguous share of the list, and the shares are placed in the one stream by two
 *  exchanges of host scalars between the ranks (any transport: gloo all-gathers in gap2seq_amd/shard.py — nothing
 *  crosses between the devices, no RCCL):
 *
 *    g2s_share_begin   the share's kernels up to its draw totals: totals[0] = draws if every draw-dependent gap took
 *                      its fewest, totals[1] = the summed spreads.          --> all ranks learn all totals
 *    g2s_share_tables  base0 / R0 = the sums of totals[0] / totals[1] over the ranks in front: the tables, and the
 *                      share's function fn[d] = deviation behind the share for deviation d in front of it, d = 0 .. R0
 *                      (*fn: valid until g2s_share_end).                    --> all ranks learn all functions
 *    g2s_share_trace   d_in = the functions of the ranks in front composed from 0: tracebacks, results, fill text.
 *    g2s_share_end     list_draws = what the whole list drew (the sum of all totals[0] + the last function's value):
 *                      this rank's generator moves past the list, as every other rank's does.
 *
 *  Every rank holds the same session state in front of the list (same seed, same lists before).  results / fill_arena:
 *  the share's own, g2s_host_alloc memory.  A share of fewer than 256 gaps, a gap with a skip rule at a share's head, a
 *  list resident mode does not take: G2S_ERR_STATE from g2s_share_begin on that rank (the caller falls back to one rank
 *  filling the list).  Results are those of g2s_fill_batch on the whole list, bit for bit (tests/test_gpu_resident.py).
 * ------------------------------------------------------------------------ */
int g2s_share_begin(g2s_session* s, const g2s_gap* gaps, size_t n, g2s_result* results, char* fill_arena, size_t arena_cap,
                    uint64_t totals[2]);
int g2s_share_tables(g2s_session* s, uint64_t base0, uint64_t R0, const uint32_t** fn);
int g2s_share_trace(g2s_session* s, uint32_t d_in);
int g2s_share_end(g2s_session* s, uint64_t list_draws);

/* ---------------------------------------------------------------------------
 *  Gap2Seq::execute() after the graph exists (Gap2Seq.cpp:224-438): scaffold
 *  scanner, per-gap statistics text, splice, FASTA text.  Outputs are malloc'ed
 *  strings released with g2s_free.  `reads_label`/`filled_label` only feed the
 *  parameter echo (Gap2Seq.cpp:180-191).
 * ------------------------------------------------------------------------ */
typedef struct g2s_run_opts {
  int32_t k, solid, max_fuz, nb_cores;
  double max_mem_gb;
} g2s_run_opts;
int g2s_execute_scaffolds(g2s_session* s, const g2s_run_opts* o, const char* reads_label,
                          const char* filled_label, const char* scaffolds_text, char** fasta, char** log,
                          int32_t* gaps, int32_t* filled);
/* The same run with the text handed over as the records are done (the reference prints a gap's statistics when
 * the gap is done, Gap2Seq.cpp:385, and appends a record to the output bank when the record is, :426-431):
 * the gaps are filled in batches of about chunk_gaps (cut at record boundaries; 0 = one batch) and after every
 * batch on_log / on_fasta receive, in input order, what that batch decided.  The concatenated text does not
 * depend on chunk_gaps. */
typedef void (*g2s_text_fn)(const char* text, size_t len, void* user);
int g2s_execute_scaffolds_stream(g2s_session* s, const g2s_run_opts* o, const char* reads_label,
                                 const char* filled_label, const char* scaffolds_text, size_t chunk_gaps,
                                 g2s_text_fn on_fasta, g2s_text_fn on_log, void* user, int32_t* gaps, int32_t* filled);
int g2s_execute_single(g2s_session* s, const g2s_run_opts* o, const char* reads_label, const char* filled_label,
                       const char* left, const char* right, int32_t length, char** fasta, char** log);
void g2s_free(void* p);

/* ---------------------------------------------------------------------------
 *  The formats either side of Gap2Seq-core in the reference's pipeline
 *  (Gap2Seq.py:294-326: GapCutter -> Gap2Seq-core -> GapMerger), host string work.
 *  g2s_cut_scaffolds: GapCutter.cpp:119-321 — scaffolds FASTA/Q text -> contigs FASTA,
 *  one-gap records FASTA (comment "<name> scaffold S contig C gap G[ split 1| split 2 k]",
 *  flanks of at most k+fuz bases), BED lines, and the tool's stdout text.
 *  g2s_merge_scaffolds: GapMerger.cpp:142-235 — contigs + (filled) gap records -> scaffolds
 *  FASTA with the markers stripped, and the tool's stdout text.
 *  The *_label arguments only feed the echoed file names.  Outputs are malloc'ed
 *  strings released with g2s_free.
 * ------------------------------------------------------------------------ */
int g2s_cut_scaffolds(const char* scaffolds_text, int k, int fuz, int mask, int no_split, const char* scaffolds_label,
                      const char* contigs_label, const char* gaps_label, const char* bed_label, char** contigs_out,
                      char** gaps_out, char** bed_out, char** log_out);
int g2s_merge_scaffolds(const char* contigs_text, const char* gaps_text, const char* scaffolds_label,
                        const char* contigs_label, const char* gaps_label, char** scaffolds_out, char** log_out);

/* ---------------------------------------------------------------------------
 *  The reference's ReadFilter (ReadFilter.cpp:344-415; called once per gap and library by Gap2Seq.py:145-149,
 *  once per library with unmapped_only by Gap2Seq.py:64-72): from a BAM file of aligned read pairs, the reads
 *  that can belong to one gap, as FASTA text (">name/1" or ">name/2", the read as sequenced).  Host work beside
 *  the fill path: BGZF/BAM are read with zlib, no index file is needed (the reference wants "<bam>.bai").
 *  fasta_out is "" when nothing was extracted (the reference then leaves no output file, Gap2Seq.py:151-153);
 *  log_out is the tool's stdout line (:406), warn_out what it writes to stderr (:188-190).  The strings are
 *  malloc'ed, released with g2s_free.  g2s_filter_last_error() describes a G2S_ERR_IO.
 * ------------------------------------------------------------------------ */
typedef struct g2s_filter_opts {
  int32_t mean_insert, std_dev;      /* -mean, -std-dev */
  int32_t breakpoint;                /* -breakpoint: 0-based position of the gap in the scaffold */
  int32_t gap_length;                /* -gap-length (default -1, as the reference's parser has it) */
  int32_t flank_length;              /* -flank-length; -1 = do not add the reads overlapping the flanks */
  int32_t unmapped_only;             /* -unmapped-only */
  int32_t threads;                   /* inflating threads; 0 = up to 8 */
  const char* scaffold;              /* -scaffold: reference sequence name in the BAM header */
} g2s_filter_opts;
int g2s_filter_reads(const char* bam_path, const g2s_filter_opts* o, char** fasta_out, char** log_out, char** warn_out,
                     int64_t* extracted, int64_t* total);
int g2s_filter_reads_mem(const void* bam_bytes, size_t n, const g2s_filter_opts* o, char** fasta_out, char** log_out,
                         char** warn_out, int64_t* extracted, int64_t* total);
const char* g2s_filter_last_error(void);

/* ---------------------------------------------------------------------------
 *  The same filter for N gaps of one library in ONE call (ABI 6, additive): two inflating passes over the BAM
 *  whatever N is, where N calls of g2s_filter_reads make 2N.  For every i, fasta_out[i], log_out[i], warn_out[i],
 *  extracted[i] and *total are what g2s_filter_reads(bam, opts_i) returns, byte for byte, opts_i being `lib` with
 *  gap i's scaffold, breakpoint, gap_length and flank_length and unmapped_only = 0 (lib's own gap fields and
 *  unmapped_only are not read; its mean_insert, std_dev and threads are).
 *
 *  Pass A keeps a compact row of every record (position, end, flag, the std::hash of its name and its mate's); the
 *  joins between rows and gaps run on the GPU `device` (readfilter_gpu.hip), or on host threads when device is -1,
 *  when that device is not a gfx950, or with G2S_HOST_FILTER=1; pass B inflates the file again to write the text of
 *  the selected reads.  Limits: fewer than 2^32 - 1 records (G2S_ERR_ARG), fewer than 2^29 gaps a call (G2S_ERR_ARG),
 *  at most 2^31 join pairs a call (G2S_ERR_NOMEM; G2S_FILTER_MAX_PAIRS lowers the cap).
 *
 *  fasta_out, log_out, warn_out: arrays of n pointers (each may be NULL), filled with malloc'ed strings released with
 *  g2s_free.  extracted: n entries, or NULL.  unmapped_out (may be NULL): the FASTA text of g2s_filter_reads with
 *  unmapped_only, every unmapped read of the file, collected in the same two passes; unmapped_extracted its count.
 *  stats may be NULL.  n = 0 is allowed (the total and the unmapped reads only).  g2s_filter_last_error() describes a
 *  failure; nothing is allocated then.
 * ------------------------------------------------------------------------ */
typedef struct g2s_filter_gap {
  const char* scaffold;              /* -scaffold */
  int32_t breakpoint, gap_length, flank_length;   /* as in g2s_filter_opts; flank_length -1 = no flank reads */
} g2s_filter_gap;
typedef struct g2s_filter_stats {
  uint32_t file_passes;              /* inflating passes over the BAM made by this call: 2, or 1 in one-pass mode, or 3
                                      * when one-pass mode's store route planned a capacity too small and started over */
  uint32_t on_device;                /* 1 when the joins ran on the GPU */
  double ms_inflate, ms_join, ms_text;   /* laps: pass A; windows and joins; pass B and the per-gap texts */
} g2s_filter_stats;
int g2s_filter_reads_gaps(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n, int device,
                          char** fasta_out, char** log_out, char** warn_out, int64_t* extracted, int64_t* total,
                          char** unmapped_out, int64_t* unmapped_extracted, g2s_filter_stats* stats);
int g2s_filter_reads_gaps_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                              size_t n, int device, char** fasta_out, char** log_out, char** warn_out, int64_t* extracted,
                              int64_t* total, char** unmapped_out, int64_t* unmapped_extracted, g2s_filter_stats* stats);

/* ---------------------------------------------------------------------------
 *  The same call handing over a POOL of reads instead of per-gap text (ABI 6, additive): every record that some gap
 *  selected, or (with want_unmapped) that is unmapped, is held ONCE, and every gap is a list of indices into the pool —
 *  what g2s_graph_build_pool takes.  The memory returned does not grow with the gaps that select a read.  Pass A, the
 *  joins and pass B are g2s_filter_reads_gaps'; so are the limits, the device rule and the errors.
 *  Contract: with names, writing ">" name "\n" bases "\n" for gap_read[gap_begin[i] .. gap_begin[i+1]) in order gives
 *  fasta_out[i] of g2s_filter_reads_gaps byte for byte (a read may be named twice by one gap, as there), and doing so
 *  for unmapped_read gives unmapped_out.  *out is written on G2S_OK only; release it with g2s_read_pool_free.
 * ------------------------------------------------------------------------ */
typedef struct g2s_read_pool {
  uint64_t n_reads;        /* distinct records held: selected by some gap, or unmapped; file order */
  char* bases;             /* the reads as sequenced, back to back, no separators */
  uint64_t* base_off;      /* [n_reads + 1] */
  char* names;             /* "name/1" or "name/2" back to back; NULL unless asked for */
  uint64_t* name_off;      /* [n_reads + 1], NULL with names */
  uint64_t* gap_begin;     /* [n + 1] */
  uint32_t* gap_read;      /* [gap_begin[n]] gap i's reads, in the order of g2s_filter_reads_gaps' fasta_out[i] */
  uint64_t n_unmapped;     /* 0 unless asked for */
  uint32_t* unmapped_read; /* [n_unmapped] ascending; an unmapped read some gap selected is the same pool entry */
} g2s_read_pool;
int g2s_filter_reads_gaps_pool(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n,
                               int device, int want_names, int want_unmapped, g2s_read_pool** out, int64_t* total,
                               g2s_filter_stats* stats);
int g2s_filter_reads_gaps_pool_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                                   size_t n, int device, int want_names, int want_unmapped, g2s_read_pool** out, int64_t* total,
                                   g2s_filter_stats* stats);
void g2s_read_pool_free(g2s_read_pool* p);

/* One-pass mode of the four batched calls above (ABI 6, additive), process-wide and atomic: 1 asks for it in every
 * later call, 0 forbids it, -1 (the initial state) follows the environment (G2S_FILTER_ONE_PASS=1|0, read per call;
 * off when it is not set).  Returns the previous mode.  One-pass mode is taken only when the joins, the inflate and
 * pass A's rows all run on the device, and then a call takes the first of three routes that fits:
 *   1. the whole stream resident: pass A leaves the inflated file in device memory and pass B is kernels that gather the
 *      selected reads from it.  Taken when the inflated file with its rows (about 2.44 times its size) fits half the free
 *      device memory (G2S_FILTER_RESIDENT_CAP=BYTES lowers that).  file_passes 1.
 *   2. the store route: the file goes through the inflate's two window slots, and pass A keeps of every record only its
 *      head, name and packed bases in one device allocation, which pass B's kernels read the same way.  Its capacities
 *      are planned from the records in the file's first MiB with a margin of a quarter, and the plan must fit the same
 *      bound.  file_passes 1 — or 3 when a planned capacity proves too small: the store is released, pass A runs again
 *      the two-pass way and pass B on the host.  (G2S_FILTER_STORE=1 takes this route even when route 1 fits, =0 never.)
 *   3. two passes: the file is inflated twice and the host walks it for pass B.  file_passes 2.
 * Outputs, messages and codes are the same bytes on every route; g2s_filter_stats::file_passes says which one ran. */
int g2s_filter_set_one_pass(int mode);

/* ---------------------------------------------------------------------------
 *  A DEVICE-HELD read pool (ABI 6, additive): g2s_filter_reads_gaps_pool with the reads' bases left where pass B made
 *  them, and the pooled build reading them there, so that a set graph is built from BAM libraries without the reads
 *  becoming host memory.  Joins, limits, codes, messages, *total and stats are g2s_filter_reads_gaps_pool's.
 *    view     a g2s_read_pool the handle owns, with bases == NULL and names == NULL; n_reads, base_off, name_off
 *             (always: callers want the lengths), gap_begin, gap_read, n_unmapped and unmapped_read equal what
 *             g2s_filter_reads_gaps_pool(..., want_names = 1, ...) returns for the same call.
 *    device   the device whose memory holds the bases, or -1 when they lie in host memory.
 *    bytes    the device bytes the handle holds.
 *    read     copies read r's base_off[r+1] - base_off[r] characters to `out` (for tests and debugging: one copy a call).
 *  The call asks for one-pass mode by itself (g2s_filter_set_one_pass(0) and G2S_FILTER_ONE_PASS=0 still forbid it).
 *  When one of the two one-pass routes ran, pass B's kernels have written the bases straight into the allocation the
 *  handle keeps, in the pooled build's layout (every read followed by one 'N', the starts as 64-bit offsets): no bases
 *  and no names are copied to the host, only offsets, lengths and index lists, and pass B's stream is synchronised before
 *  the call returns.  On every other route (two passes, the host walk, device -1, no gfx950, G2S_HOST_FILTER,
 *  G2S_HOST_ROWS, G2S_HOST_INFLATE, a store overflow, a failed allocation) the handle is host-held, with the same
 *  contents; a caller never has to care which kind it got.  *out is written on G2S_OK only.
 *  g2s_device_pool_free sets the handle's device before it frees.  A build keeps no pointer into a pool: pools may be
 *  freed while graphs built from them live.
 * ------------------------------------------------------------------------ */
typedef struct g2s_device_pool g2s_device_pool;
int g2s_filter_reads_gaps_dpool(const char* bam_path, const g2s_filter_opts* lib, const g2s_filter_gap* gaps, size_t n,
                                int device, int want_unmapped, g2s_device_pool** out, int64_t* total, g2s_filter_stats* stats);
int g2s_filter_reads_gaps_dpool_mem(const void* bam_bytes, size_t nbytes, const g2s_filter_opts* lib, const g2s_filter_gap* gaps,
                                    size_t n, int device, int want_unmapped, g2s_device_pool** out, int64_t* total,
                                    g2s_filter_stats* stats);
const g2s_read_pool* g2s_device_pool_view(const g2s_device_pool* p);
int g2s_device_pool_device(const g2s_device_pool* p);
uint64_t g2s_device_pool_bytes(const g2s_device_pool* p);
int g2s_device_pool_read(const g2s_device_pool* p, uint64_t r, char* out);
void g2s_device_pool_free(g2s_device_pool* p);
/* g2s_graph_build_pool_reach over such pools: read r of pools[p] has index first[p] + r, first[p] being the sum of n_reads
 * over the earlier pools; every other argument, the argument errors (an index >= the pools' total, npools == 0, exactly
 * one reach array NULL: G2S_ERR_ARG, *out not written) and the graph are g2s_graph_build_pool_reach's on the sequences
 * the pools hold (both reach arrays NULL: g2s_graph_build_pool's).  The device build copies the reads in use that lie in
 * a pool held on its device into its text device to device; reads of a host-held pool, or of a pool on another device,
 * are packed on the host and uploaded, their share of the text only.  The host build (no device, G2S_HOST_BUILD=1, the
 * device build giving up, and one set without reach records, which is an ordinary graph build) copies a device-held
 * pool's text down once a call. */
int g2s_graph_build_dpool_reach(const g2s_device_pool* const* pools, uint32_t npools, const uint64_t* set_begin,
                                const uint32_t* set_seq, const uint32_t* shared_seq, uint64_t nshared,
                                const uint8_t* set_shared, uint32_t nsets, int k, int solid, int nthreads,
                                const struct g2s_gap* reach_gap, const int32_t* reach_radius, g2s_graph** out);

/* The chunked device inflate of plain gzip read files (ABI 6, additive), process-wide and atomic: 1 asks for it in every
 * later g2s_graph_build_files, 0 forbids it, -1 (the initial state) follows the environment (G2S_DEVICE_GZIP=1|0, read
 * per call; off when it is not set).  Returns the previous mode.  With it a read file that is gzip but no BGZF file (a
 * .fq.gz as gzip(1) writes it) is inflated on the device from many places of its deflate stream at once
 * (csrc/gzip_inflate.h) instead of by one zlib stream on the host.  The route completes a file only when every chunk
 * ended at the block start the next one began at and every member's CRC-32 and ISIZE matched; on anything else the file
 * is read again from its first byte by zlib, so texts, counts, errors and messages are the same bytes either way.
 * G2S_HOST_READS=1, G2S_HOST_INFLATE=1, G2S_HOST_BUILD, pipes and a missing device keep their routes.
 * G2S_GZIP_CHUNK_BYTES, G2S_GZIP_WINDOW_CHUNKS and G2S_GZIP_SLOT_RATIO size it (README). */
int g2s_reads_set_device_gzip(int mode);

/* ---------------------------------------------------------------------------
 *  Page-locked host memory the GPUs can write: a `results` array or fill arena
 *  allocated here is written by the kernels directly (no staging copy) when a
 *  list is finished on the device.  Any other memory works too.  The reference's
 *  caller allocates `fill` with new[] (Gap2Seq.cpp:374).
 * ------------------------------------------------------------------------ */
void* g2s_host_alloc(size_t bytes);
void g2s_host_free(void* p);

/* Accessors. */
const g2s_graph* g2s_session_graph(const g2s_session* s);
int g2s_session_get_params(const g2s_session* s, g2s_params* out);

/* (The g2s_test_* entry points the unit tests call are declared in include/g2s_test.h: they are not part of the
 * reference-facing interface.) */

/* Checks the invariants the kernels rely on between the unitig-start bitmap and
 * the successor table (every edge the bitmap calls unitig-internal is the only edge out of
 * its source and the only edge into its target, in both orientations; the last-base table
 * agrees with the successor slots).  Returns the number of violations found (0 = consistent)
 * and describes the first few in msg (NUL-terminated, at most msg_cap bytes). */
int64_t g2s_graph_validate(const g2s_graph* g, char* msg, size_t msg_cap);

/* Number of usable gfx950 devices (0 when none / no driver). */
int g2s_device_count(void);

/* ---------------------------------------------------------------------------
 *  Synthetic workloads of BASELINE.md / SURVEY.md §8(d) (seeded, generator
 *  lives here so that bench.py, the tests and the CLI agree byte for byte).
 *  variant bit 0: plant repeats (V1), bit 1: second haplotype with one
 *  substitution every ~500 bp (V2).  Returns malloc'ed FASTA texts.
 * ------------------------------------------------------------------------ */
int g2s_synth_genome(uint64_t length, uint32_t variant, uint64_t seed, char** reads_fasta);
int g2s_synth_gaps(const char* reads_fasta, int k, int fuz, int ngaps, int min_len, int max_len, uint64_t seed,
                   char** scaffolds_fasta);

#ifdef __cplusplus
}
#endif
#endif /* G2S_H_ */
