/* include/g2s_test.h — TEST HOOKS of libg2s_hip.so, kept apart from the reference-facing C ABI (include/g2s.h).
 *
 * Nothing here is a fill path (none of these can compute the DP) and nothing of the reference binds to them: they let
 * the unit tests (tests/test_host.py, tests/test_seg_model.py, tests/test_shard.py, tests/test_gpu_*.py) drive single
 * pieces of the host side — the host half of phase D on caller-supplied tables, the graph tables, the rand() stream
 * of the host and of the device, the worker pool, the shared group counter — without a kernel run; and one drives the
 * joins of the batched read filter (host or device) on rows and windows instead of a BAM file. */
#ifndef G2S_TEST_H_
#define G2S_TEST_H_
#include "g2s.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 *  TEST HOOK (CPU unit tests of the host half of phase D only; not a fill
 *  path: it cannot compute the DP).  Runs D1/D2/D3 for ONE gap on a DP table
 *  supplied by the caller: n_states states (oriented node, depth, count) plus
 *  the phase C outcome.  The rand() stream is srand(seed) advanced by `skip`
 *  draws.  `buf` needs gap_len + k + d_err + lmf + rmf + 3 bytes.
 * ------------------------------------------------------------------------ */
int g2s_test_post_gap(const g2s_graph* g, const g2s_params* p, const g2s_gap* gap, int32_t n_states,
                      const uint32_t* nodes, const int32_t* depths, const uint32_t* counts, int32_t c_count,
                      int32_t n_lengths, const int32_t* lengths, int32_t reached_j, int32_t final_d, uint32_t seed,
                      uint32_t skip, g2s_result* res, char* buf);

/* TEST HOOK: the host half of phase D (D2 + D3) on a backward closure supplied by the caller in
 * the layout the kernels emit: n records of 16 bytes {node, count, depth | flags << 27, first
 * parent index | G2S more-parents bit, or -1} in an order in which every parent comes AFTER its
 * children, plus the side list of further parents (state << 32 | parent).  Used by the CPU
 * tests of the kernel's algorithm model (tests/seg_model.py); cannot compute the DP. */
int g2s_test_post_closure(const g2s_graph* g, const g2s_params* p, const g2s_gap* gap, uint32_t n_records,
                          const uint32_t* records /* 4 words each */, uint32_t n_xp, const uint64_t* xp, int32_t c_count,
                          int32_t n_lengths, const int32_t* lengths, int32_t reached_j, int32_t final_d, uint32_t seed,
                          uint64_t skip, g2s_result* res, char* buf);

/* TEST HOOK: the host half of phase D run directly on closure segments (the segment tier's output,
 * layout as for g2s_test_seg_expand), as the batch path does when no k-mer occurs at two depths of
 * the closure; *on_segments = 0 when that does not hold (nothing is computed then: take
 * g2s_test_seg_expand + g2s_test_post_closure, as the batch path does). */
int g2s_test_post_segments(const g2s_graph* g, const g2s_params* p, const g2s_gap* gap, uint32_t n_segs,
                           const uint32_t* segs, int32_t c_count, int32_t n_lengths, const int32_t* lengths,
                           int32_t reached_j, int32_t final_d, uint32_t seed, uint64_t skip, g2s_result* res, char* buf,
                           int32_t* on_segments);

/* TEST HOOK: the host's expansion of a closure given as unitig segments (what the segment tier's
 * kernel emits: 8 words per segment {node, depth | len << 16, count, ts | tt << 16, parents 0-1,
 * parents 2-3, flags, 0}, children before parents) into the per-state records and side list of
 * g2s_test_post_closure.  n_records / n_xp must be the exact output sizes. */
int g2s_test_seg_expand(const g2s_graph* g, const g2s_params* p, const g2s_gap* gap, uint32_t n_segs,
                        const uint32_t* segs, int32_t n_lengths, const int32_t* lengths, int32_t reached_j,
                        uint32_t n_records, uint32_t* records, uint32_t n_xp, uint64_t* xp);

/* TEST HOOK: copies of the tables the kernels walk: the successor table (2 * kmers * 4 words,
 * G2S_INVALID_NODE = none) and the unitig-start bitmap ((kmers + 63) / 64 words; bit i set = the
 * edge 2(i-1) -> 2i is not unitig-internal). */
int g2s_test_graph_tables(const g2s_graph* g, uint32_t* succ_out, uint64_t* ustart_out);

/* TEST HOOK: values [skip, skip+n) of the session-style rand() stream after srand(seed)
 * (the flat glibc TYPE_3 generator the tracebacks read), for comparison with libc. */
int g2s_test_rand_stream(uint32_t seed, uint32_t skip, uint32_t n, int32_t* out);

/* TEST HOOK: the same values reached by a JUMP over the `skip` values in front (the recurrence's polynomial: what
 * g2s_share_end moves a rank's generator with when the values were drawn on other ranks' devices). */
int g2s_test_rand_skip(uint32_t seed, uint64_t skip, uint32_t n, int32_t* out);

/* TEST HOOK: the same values from the DEVICE's generator (d3_device.hip: g2s_rand_fill — the state behind `skip`
 * values handed over by the host, every block of 4096 values reached with three jump polynomials). */
int g2s_test_device_rand(int device, uint32_t seed, uint64_t skip, uint32_t n, int32_t* out);

/* TEST HOOK: the product's kernel g2s_d3_tables_waves (d3_device.hip, a short list's tables: the draws of a draw-dependent gap's traceback for every
 * place of the list's rand() stream it can start at) for ONE gap of the caller's design, on `device`.  segs: n_segs closure
 * segments of four words {depth | len << 16, parents 0-1, parents 2-3, flags} (a parent slot without a parent: 0xFFFF);
 * n_len (1 or 2) path lengths len0 / len1 and their start segments start_seg = start 0 | start 1 << 16; rnd: rnd_cap raw
 * words of the stream from its first value (rand() = word >> 1; nothing exists behind them); base: the gap's first draw
 * at deviation 0; R: its deviations are 0 .. R; dmin / dspread: its fewest draws and most - fewest.  entries[d] receives
 * what the kernel wrote to the table (draws - dmin, or 0 for a bad walk), bad[d] whether the walk was bad, for d in
 * [0, R]; *anomalies the list's anomaly counter (nonzero = the list would go to the host path). */
int g2s_test_d3_tables(int device, const uint32_t* segs, uint32_t n_segs, int32_t n_len, int32_t len0, int32_t len1,
                       uint32_t start_seg, const uint32_t* rnd, uint64_t rnd_cap, uint32_t base, uint32_t R, uint32_t dmin,
                       uint32_t dspread, uint16_t* entries, uint8_t* bad, uint32_t* anomalies);

/* TEST HOOK: how many lists of this process took phase D3's short route: no g2s_d3_back between the tables' kernel and
 * the trace kernel, whose workgroups walk the offsets' chain themselves (lists of up to 768 gaps on one session, not a
 * set list, not in flight; G2S_D3_BACK=1 keeps every list off it). */
uint64_t g2s_test_d3_chain_launches(void);

/* TEST HOOK: the host worker pool that runs the per-gap analysis and tracebacks: `rounds`
 * parallel-for rounds of `n` tasks on `threads` threads (task i adds i+1 to a per-round
 * sum); returns G2S_OK when every task of every round ran exactly once. */
int g2s_test_worker_pool(int32_t threads, int32_t rounds, int32_t n);

/* TEST HOOK: the shared group counter g2s_team_fill's sessions pull from, with `nworkers`
 * host threads in place of sessions: owner[i] receives the worker that was handed gap i.
 * G2S_OK when every gap of [0, n) was handed out exactly once, in contiguous groups. */
int g2s_test_group_queue(int32_t nworkers, uint64_t n, uint64_t group_size, int32_t* owner);
/* The same with one worker that needs slow_us microseconds more for every group it takes than the others (a busy
 * or slower device): what it does not get to is taken by the others — the queue hands a group to whoever asks. */
int g2s_test_group_queue_slow(int32_t nworkers, uint64_t n, uint64_t group_size, int32_t slow_worker, uint32_t slow_us,
                              int32_t* owner);

/* TEST HOOK: the joins of the batched read filter (readfilter_gaps.hpp: FilterRows, FilterJoin) on rows and windows
 * supplied by the caller, without a BAM file: nr rows (reference, position, end position, flag, hash of the own name
 * and of the mate's), the longest span, the filter's size in bits, n gaps with three windows each (`windows`: 9 values
 * a gap, (tid, beg, end) of the left, the right and the flank window) and the pair cap.  device < 0: filter_join_host
 * on `threads` threads; device >= 0: filter_join_device on that device — G2S_ERR_NO_DEVICE when it is no usable
 * gfx950 (never the host path in its place; G2S_HOST_FILTER is not read).  Returns the join's own code, its message in
 * g2s_filter_last_error().  *n1 / *n2 receive the true sizes of list 1 / list 2 ((gap << 32 | row), ascending); the
 * first min(cap, size) pairs of each are written, so a caller whose capacity was too small calls again. */
int g2s_test_filter_join(int device, int32_t threads, uint64_t nr, const int32_t* ref_id, const int32_t* pos,
                         const int64_t* end, const uint32_t* flag, const uint64_t* h_own, const uint64_t* h_mate,
                         int64_t max_span, uint64_t bits, uint64_t n, const int64_t* windows, uint64_t max_pairs,
                         uint64_t* list1, uint64_t cap1, uint64_t* n1, uint64_t* list2, uint64_t cap2, uint64_t* n2);

/* TEST HOOK: what the process's last g2s_graph_build_pool of several sets did.  own_positions: bases + 1 of every
 * occurrence of a sequence in the sets' own lists; shared_positions: the same of the shared list, once (0 when no set
 * is flagged); keys_sorted: the keys that went through a sort.  On the device (*on_device = 1) keys_sorted ==
 * own_positions + shared_positions whatever the number of flagged sets: the shared list is sorted once.  The host
 * build (*on_device = 0) works on every set's expanded list: own_positions + flagged sets * shared_positions.  Any
 * pointer may be NULL. */
int g2s_test_last_pool_build(uint64_t* own_positions, uint64_t* shared_positions, uint64_t* keys_sorted, int* on_device);

/* TEST HOOK: the device-held read pools (g2s.h: g2s_device_pool).  Of the process's last g2s_filter_reads_gaps_dpool[_mem]:
 * held_on_device, 1 when the handle it returned holds its bases in device memory, and bases_bytes_to_host, the bytes of
 * bases that became host memory in that call (0 for a device-held handle).  Of the process's last pooled build
 * (g2s_graph_build_pool[_reach], g2s_graph_build_dpool_reach): the positions (bases + 1) of the sequences in use, once
 * each, that the device build copied from a device-held pool (text_bytes_gathered_on_device) and that went through host
 * memory (text_bytes_packed_on_host; the host build: all of them).  Any pointer may be NULL. */
int g2s_test_last_dpool(int* held_on_device, uint64_t* bases_bytes_to_host, uint64_t* text_bytes_gathered_on_device,
                        uint64_t* text_bytes_packed_on_host);

/* TEST HOOK: what the process's last single-graph build (g2s_graph_build_files / g2s_graph_build_seqs) did for its solid
 * k-mer set.  positions: bases + 1 of every sequence; passes: the key-range passes that ran on the device (0: the
 * one-sort device count, or the host count); refined_bins: the histogram bins that held more than a pass's keys and were
 * histogrammed again on their next bits; max_pass_keys: the keys of the largest pass (never more than
 * G2S_BUILD_PASS_KEYS); solid: the solid k-mers found; on_device: the set was made on the device (0 also when the
 * device count gave up and the host count took over).  Any pointer may be NULL. */
int g2s_test_last_solid_count(uint64_t* positions, uint32_t* passes, uint32_t* refined_bins, uint64_t* max_pass_keys,
                              uint64_t* solid, int* on_device);

/* TEST HOOK: the graph build's text of ONE read file in memory (FASTA or FASTQ, plain, gzip or BGZF, recognised by its
 * magic bytes): every sequence followed by one 'N'.  device == -1: the host loader — zlib when the bytes are gzip, then
 * parse_fastx.  device == -2: the line state machine of csrc/fastx_machine.h, the one the kernels run, walked line by line
 * on the host.  device >= 0: the kernels k_fastx_* of csrc/reads_text.hip on that device, in pieces of piece_bytes raw
 * bytes (0: the product's choice, 32 MiB at most), BGZF members inflated on the device unless G2S_HOST_INFLATE=1 —
 * G2S_ERR_NO_DEVICE when it is no usable gfx950, G2S_ERR_HIP when anything on the device refuses; never the host in
 * their place.  The bytes of a BAM file give the BAM text (include/g2s.h): device == -1 and -2 by the reader's walk (there
 * is no line machine for BAM), device >= 0 by the kernels k_bamreads_* of csrc/bam_reads.hip, piece_bytes being the
 * window — by k_bamstream_*, the streaming form, when the file is over G2S_BUILD_RESIDENT_CAP or
 * G2S_BUILD_BAM_STREAM=1 asks for it (both are read here as g2s_graph_build_files reads them) —; with
 * G2S_HOST_INFLATE=1 by the reader's walk, copied up.
 * G2S_ERR_IO with g2s_last_error()'s text for a truncated or corrupt gzip stream.  *out_n receives the
 * text's size; the first min(cap, size) bytes are written, so a caller whose capacity was too small calls again.
 * g2s_test_last_reads_load then speaks of this call. */
int g2s_test_reads_text(const void* bytes, size_t n, int device, size_t piece_bytes, uint8_t* out, size_t cap, size_t* out_n);

/* TEST HOOK: how the process's last g2s_graph_build_files (or g2s_test_reads_text) loaded its reads.  files; raw_bytes:
 * the files' bytes after inflation; positions: the text's (bases + 1 a record); records; pieces: the pieces the kernels
 * walked (0 on the host); on_device: the text was made by the kernels (0 also when the device loader or the device
 * count gave up and the host loader took over); inflate[i] for the first min(inflate_cap, files) files: 0 not compressed,
 * 1 zlib on the host, 2 BGZF members inflated on the device, 3 both (BGZF members first, then another gzip stream),
 * 4 a plain gzip stream inflated chunk by chunk on the device (only when asked for: g2s_reads_set_device_gzip);
 * grows: how often the text buffer was enlarged.  Any pointer may be NULL. */
int g2s_test_last_reads_load(uint64_t* files, uint64_t* raw_bytes, uint64_t* positions, uint64_t* records, uint64_t* pieces,
                             int* on_device, int* inflate, uint64_t inflate_cap, uint64_t* grows);

/* TEST HOOK: the BAM files (csrc/bam_reads.h) among the read files of the process's last g2s_graph_build_files (or
 * g2s_test_reads_text).  bam_files; kept / skipped: their records that gave a sequence / that were secondary or
 * supplementary; by_kernels: 1 when k_bamreads_* or k_bamstream_* wrote the text of every one of them; reason, when they did not:
 * 0 the kernels wrote it, 1 not asked (G2S_HOST_BUILD, G2S_HOST_READS=1, G2S_HOST_INFLATE=1, no usable device, or the
 * host loader took over for another reason), 2 the row kernels gave a file back — *anomaly is then the RowsAnomaly of
 * csrc/bam_rows.h —, 3 over half the free device memory or G2S_BUILD_RESIDENT_CAP: stream, rows and text, and the
 * streaming form's windows and text too (or its text outgrew what the bound left), 4 an allocation or a HIP call
 * failed.  Any pointer may be NULL. */
int g2s_test_last_reads_bam(uint64_t* bam_files, uint64_t* kept, uint64_t* skipped, int* by_kernels, int* reason, int* anomaly);

/* TEST HOOK: the streaming form of the BAM read route (csrc/bam_reads.h) in the process's last g2s_graph_build_files (or
 * g2s_test_reads_text).  streamed_files: the BAM files whose text k_bamstream_* wrote window by window (a file that is
 * resident, or that the host loader read, counts 0); windows: the walk windows those files took (they are among
 * g2s_test_last_reads_load's pieces); peak_device_bytes: the largest footprint counted against the bound of half the
 * free device memory and G2S_BUILD_RESIDENT_CAP for one of them — the inflate's two slots with their fronts, the
 * candidate and ring arrays, the lengths with the scan's scratch, and the text buffer's capacity, each as the bytes
 * asked of the allocator (its granularity is not counted, nor are the loader's own raw buffers for the FASTA/FASTQ files
 * of the list — as for the resident route).  All 0 when no file was streamed.  Any pointer may be NULL. */
int g2s_test_last_reads_bam_stream(uint64_t* streamed_files, uint64_t* windows, uint64_t* peak_device_bytes);

/* TEST HOOK: the planner of the key-range passes (pass_plan.hpp) on a histogram of the caller's: nbins consecutive bins
 * of the key space, cut greedily and in order into passes of at most cap keys — a pass is closed in front of the first
 * bin that would take it beyond cap, empty bins join the open pass.  *npasses receives the number of passes and
 * first_bin_of_pass[p] the first bin of pass p for p < min(*npasses, max_passes) (pass p ends where pass p + 1 begins,
 * the last one at nbins).  A bin with more than cap keys stands alone in its pass; *first_oversized_bin (may be NULL)
 * receives the first such bin, or nbins when there is none. */
int g2s_test_plan_passes(const uint64_t* hist, uint32_t nbins, uint64_t cap, uint32_t* first_bin_of_pass,
                         uint32_t max_passes, uint32_t* npasses, uint32_t* first_oversized_bin);

/* TEST HOOK: what the process's last bounded single-graph build (g2s_graph_build_seqs_reach / _files_reach taking the
 * bounded path) did: the records, their seeds, the seeds that are solid k-mers (counted with their copies), the k-mers
 * of the full and of the kept set, the key-range passes that made the device-held table (0: one sort, or the host), how
 * often the search started over with a larger queue, whether it ran on the device, and the wall time of the level loop.
 * levels differs by path: on the host the last level with a frontier; on the device the level at which the loop
 * stopped — the largest radius, or, when the search died out earlier, the level of the control read that saw it, up to
 * 7 behind the host's figure.  Compare it between the paths only where the search runs to the largest radius. */
int g2s_test_last_graph_reach(uint64_t* records, uint64_t* seeds, uint64_t* seeds_in_full, uint64_t* full_kmers,
                              uint64_t* kept_kmers, uint32_t* levels, uint32_t* passes, uint32_t* regrowths, int* on_device,
                              double* ms_search);
/* TEST HOOK: what the process's last g2s_graph_build_pool_reach with at least one reach record did.  reach_sets: the
 * sets with a record; full_kmers: the k-mers of those sets' full graphs, valid when *full_known != 0 (the host build
 * counts them when it was the first choice — no device, G2S_HOST_BUILD=1; the device build never forms the
 * full graphs and does not count them, nor does the host build behind a device build that gave up); kept_kmers: the
 * k-mers those sets hold in the graph; levels: the deepest level any set's search ran (0: seeds only; never more than
 * the largest radius); on_device: the search ran in the device kernel.  Any pointer may be NULL. */
int g2s_test_last_pool_reach(uint64_t* reach_sets, uint64_t* full_kmers, int* full_known, uint64_t* kept_kmers,
                             uint32_t* levels, int* on_device);

/* The record the segment tier's kernels read when they walk BACKWARDS from the oriented node `node` of a graph on
 * `device` (the graph is uploaded and its tables are built if they are not there yet): out[0..3] = the predecessors, in
 * slot order and each with its orientation bit flipped (G2S_INVALID_NODE stays), of the node b at which the
 * unitig-internal walk back from `node` ends; out[4] = the steps of that walk.  At odd k this is the forward record of
 * node ^ 1; at even k it comes from the explicit predecessor table, and for either id of a palindromic k-mer b is the
 * palindrome's one node. */
int g2s_test_seg_back_record(g2s_graph* g, int device, uint32_t node, uint32_t out[5]);

/* TEST HOOK: a whole BGZF file (any members, no BAM header needed) inflated by one of the reader's three inflaters
 * (bam.cpp), through the reader's windows (G2S_BAM_CHUNK).  device >= 0: the kernel g2s_bgzf_inflate on that device —
 * G2S_ERR_NO_DEVICE when it is no usable gfx950, G2S_ERR_HIP when it refuses later; never the host in its place.
 * device == -1: zlib, the product's host path.  device == -2: csrc/inflate_core.h, the kernel's decoder and its CRC by
 * slices, compiled for the host, one member after another.  G2S_OK, or G2S_ERR_IO with g2s_filter_last_error()'s text
 * and, when a member is corrupt, its index in *bad_member (else -1).  *out_n receives the inflated size; the first
 * min(cap, size) bytes are written, so a caller whose capacity was too small calls again. */
int g2s_test_bgzf_inflate(const void* bytes, size_t n, int device, uint8_t* out, size_t cap, size_t* out_n,
                          int64_t* bad_member);

/* TEST HOOK: what the reader did in the process's last g2s_filter_reads_gaps[_mem] / _pool[_mem] call: whether every
 * window of both passes was inflated on the device, the members and bytes in and out of both passes together, and per
 * pass the time spent inside the reader's refills (with the device's look-ahead: what the record walk waited).  Any
 * pointer may be NULL. */
int g2s_test_last_filter_inflate(int* on_device, uint64_t* members, uint64_t* bytes_in, uint64_t* bytes_out,
                                 double* ms_pass_a_inflate, double* ms_pass_b_inflate);

/* TEST HOOK: pass A of the batched read filter alone, on a BAM file in memory: one row per record in file order
 * (reference, position, end position, flag, hash of the own name and of the mate's), the record count, the longest
 * l_seq and the longest span of a record with a reference (1 when there is none).  device == -1: the host walk
 * (BamFile::for_each).  device >= 0: the kernels of csrc/bam_rows.hip behind the device inflate — G2S_ERR_NO_DEVICE when
 * it is no usable gfx950, G2S_ERR_HIP when the kernels refuse or meet an anomaly (g2s_test_last_filter_rows says
 * which); never the host walk in their place, and no switch is read.  `window`: the bytes the kernels walk at a time;
 * 0 = a whole window of inflated members (G2S_BAM_CHUNK), and smaller values cut that window further.  The first
 * min(cap, *total) rows are written, so a caller whose capacity was too small calls again.  A file the host walk
 * rejects is G2S_ERR_IO with its message in g2s_filter_last_error(). */
int g2s_test_bam_rows(const void* bytes, size_t n, int device, size_t window, uint64_t cap, int32_t* ref_id, int32_t* pos,
                      int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate, uint64_t* total, int32_t* read_length,
                      int64_t* max_span);

/* TEST HOOK: g2s_test_bam_rows with pass A as one-pass mode runs it on a device (csrc/bam_text.h): every window inflated
 * to its place in one device allocation, the row kernels on the word boundary in front of it, the chain's head moved from
 * window to window in place of the carry.  The rows must be g2s_test_bam_rows'.  G2S_ERR_HIP also when the stream was not
 * kept (over the cap, a failed allocation); device == -1 is the host walk, as there. */
int g2s_test_bam_rows_kept(const void* bytes, size_t n, int device, size_t window, uint64_t cap, int32_t* ref_id, int32_t* pos,
                           int64_t* end, uint32_t* flag, uint64_t* h_own, uint64_t* h_mate, uint64_t* total,
                           int32_t* read_length, int64_t* max_span);

/* TEST HOOK: the hash of the name bytes[0 .. strnlen(bytes, len)) followed by "/1" or "/2" (`which`: 1 or 2; len at
 * most 255): *std_hash from std::hash<std::string>, as the host walk takes it, and *own_hash from the host compilation
 * of csrc/name_hash.h, the function the kernels run. */
int g2s_test_name_hash(const void* bytes, size_t len, int which, uint64_t* std_hash, uint64_t* own_hash);

/* TEST HOOK: what pass A did in the process's last g2s_filter_reads_gaps[_mem] / _pool[_mem] call, or in the last
 * g2s_test_bam_rows: whether its rows were made on the device, the windows the kernels walked, the records, the
 * candidate record starts the kernels flagged (0 for a host walk), and the anomaly (csrc/bam_rows.h: RowsAnomaly; 0 =
 * none) that handed the pass to the host walk: 1 a dead link of the chain, 2 more candidates than a window's capacity,
 * 3 a carried record head longer than the room in front of a window, 4 a chain that does not end at the stream's end,
 * 5 an allocation or a HIP call failed, 6 name_hash.h is not this build's std::hash, 7 a member did not inflate, 8 a
 * file outside the kernels' limits.  Any pointer may be NULL. */
int g2s_test_last_filter_rows(int* on_device, uint64_t* windows, uint64_t* records, uint64_t* candidates, int* anomaly);

/* TEST HOOK: what pass B did in the process's last g2s_filter_reads_gaps[_mem] / _pool[_mem] call.  *one_pass: 1 when it
 * ran on the device from the stream pass A kept there (one-pass mode, g2s_filter_set_one_pass); *reason why it did not
 * (csrc/bam_text.h: TextReason): 0 it did, 1 not asked for, 2 pass A's rows were not made on the device (no device, a
 * switch, an anomaly), 3 the inflated file and its rows are over the cap (half the free device memory,
 * G2S_FILTER_RESIDENT_CAP) and so is the store route's need (or G2S_FILTER_STORE=0), 4 an allocation or a HIP call
 * failed, 5 a capacity the store route planned from the file's sample was too small: pass A ran again the two-pass way
 * and pass B on the host (file_passes 3).  *reads / *bytes: the records pass B's kernels produced and the bytes of their
 * bases, names or text (0 when it did not run there); *resident_bytes: the inflated stream pass A kept on the device,
 * or on the store route the store's used bytes, which are fewer than the inflated file's (0: none).  Any pointer may be
 * NULL. */
int g2s_test_last_filter_text(int* one_pass, int* reason, uint64_t* reads, uint64_t* bytes, uint64_t* resident_bytes);

/* TEST HOOK: pass B of the batched read filter alone, on a BAM file in memory, for the records whose indices (in file
 * order, from 0) are rows[0 .. n_rows) — in any order, repeats allowed; a row beyond the file's records is G2S_ERR_ARG.
 * device == -1: the host walk (BamFile::for_each with append_bases / own_name).  device >= 0: pass A's kernels with the
 * inflated file kept on the device, then the kernels of csrc/bam_text.hip — G2S_ERR_NO_DEVICE when it is no usable
 * gfx950, G2S_ERR_HIP when anything on the device refuses; never the host walk in their place.
 * fasta == 0: the pool's arrays for the selected records in file order: their bases back to back with base_off, and with
 * want_names their names (name, "/1" or "/2") back to back with name_off.  fasta != 0: `bases` receives the records'
 * FASTA texts (">" name "/1|/2" "\n" bases "\n") back to back and base_off where each begins; no names.
 * *n_reads: the distinct selected records; base_off / name_off have *n_reads + 1 entries, of which the first
 * min(off_cap, *n_reads + 1) are written; *bases_n / *names_n are the true sizes and the first min(cap, size) bytes are
 * written, so a caller whose capacity was too small calls again. */
int g2s_test_bam_text(const void* bytes, size_t n, int device, const uint32_t* rows, uint64_t n_rows, int want_names, int fasta,
                      uint8_t* bases, uint64_t bases_cap, uint64_t* bases_n, uint8_t* names, uint64_t names_cap,
                      uint64_t* names_n, uint64_t* base_off, uint64_t* name_off, uint64_t off_cap, uint64_t* n_reads);

/* TEST HOOK: g2s_test_bam_text with pass A in store form on a device (csrc/bam_store.h): the file through the inflate's two
 * slots, the row kernels `window` bytes at a time (0: a whole window of inflated members), the store's kernels behind
 * them, and pass B's kernels on the store.  The capacities are the ones that cannot overflow; no switch is read.
 * G2S_ERR_HIP when the store was not made; device == -1 is the host walk, as there. */
int g2s_test_bam_text_store(const void* bytes, size_t n, int device, size_t window, const uint32_t* rows, uint64_t n_rows,
                            int want_names, int fasta, uint8_t* bases, uint64_t bases_cap, uint64_t* bases_n, uint8_t* names,
                            uint64_t names_cap, uint64_t* names_n, uint64_t* base_off, uint64_t* name_off, uint64_t off_cap,
                            uint64_t* n_reads);

/* TEST HOOK: the store route's plan (csrc/bam_store.h: store_plan) for a BAM file in memory; needs no device.  The sample
 * is the records that begin in the first 1 MiB (G2S_FILTER_STORE_SAMPLE=BYTES) of the inflated stream behind the
 * header, or in the whole file when it is smaller: *sample_records records over *sample_bytes bytes (the last one
 * whole, so the bytes may reach beyond the sample's end) with *sample_stored stored bytes.  With P the inflated bytes
 * behind the header, *rows_cap = min(P / 36 + 1, ceil(1.25 r / z P) + 64), *store_cap = min(P, ceil(1.25 c / z P) +
 * 4096), *need = 52 (rows_cap + 1) + store_cap.  Any pointer may be NULL. */
int g2s_test_filter_store_plan(const void* bytes, size_t n, uint64_t* sample_records, uint64_t* sample_bytes,
                               uint64_t* sample_stored, uint64_t* rows_cap, uint64_t* store_cap, uint64_t* need);

/* TEST HOOK: the store of a BAM file in memory (csrc/bam_store.h): of every record in file order the 36 head bytes with
 * block_size rewritten to 32 + l_name + ceil(l_seq / 2) and n_cigar_op to 0, the l_name name bytes and the packed
 * bases, back to back; rec_off[i] is where record i begins.  device == -1: the host model (bam_store::append_record
 * under BamFile::for_each).  device >= 0: the kernels of csrc/bam_store.hip behind the device inflate and the row
 * kernels, `window` bytes at a time — G2S_ERR_NO_DEVICE when it is no usable gfx950, G2S_ERR_HIP when anything on the
 * device refuses; never the host in their place, and no switch is read.  *store_n / *n_records are the true sizes; the
 * first min(store_cap, *store_n) bytes and min(off_cap, *n_records) offsets are written, so a caller whose capacity was
 * too small calls again. */
int g2s_test_bam_store(const void* bytes, size_t n, int device, size_t window, uint8_t* store, uint64_t store_cap,
                       uint64_t* store_n, uint64_t* rec_off, uint64_t off_cap, uint64_t* n_records);

/* TEST HOOK: the store route in pass A of the process's last g2s_filter_reads_gaps[_mem] / _pool[_mem] call.  *used: 1
 * when pass B read the store; *records / *store_bytes: what the store held; *store_cap / *rows_cap: the planned
 * capacities (0: no plan was made); *device_bytes: the plan's need, counted against the bound of half the free device
 * memory and G2S_FILTER_RESIDENT_CAP; *overflow: 0 none, 1 the planned rows, 2 the planned store.  Any pointer may be
 * NULL. */
int g2s_test_last_filter_store(int* used, uint64_t* records, uint64_t* store_bytes, uint64_t* store_cap, uint64_t* rows_cap,
                               uint64_t* device_bytes, int* overflow);

/* TEST HOOK: a whole gzip file (any members; no BGZF needed) inflated by one of three inflaters, in chunks of chunk_bytes
 * compressed bytes (0: G2S_GZIP_CHUNK_BYTES or the default) and windows of window_chunks chunks (0: the whole file in
 * one window).  device >= 0: the kernels of csrc/gzip_inflate.hip on that device — G2S_ERR_NO_DEVICE when it is no
 * usable gfx950, G2S_ERR_HIP when it refuses; never the host in their place.  device == -1: zlib, the product's host
 * path.  device == -2: csrc/gzip_chunks.h, the kernels' algorithm, compiled for the host, chunk by chunk.  For -2 and
 * the kernels *outcome (may be NULL) receives why the route gave the file back (csrc/gzip_inflate.h: GzipOutcome) — 0 it
 * did not, 1 too few starts (a window that does not reach the file's end found no second start; the loader's rule of a
 * quarter of the chunks is not applied here), 2 boundary mismatch, 3 slot full, 4 corrupt, 5 a member's CRC-32, ISIZE or
 * cut trailer, 6 memory, 8 a member header — and then *out_n is 0 and no byte is written: G2S_OK all the same.
 * device == -1 gives G2S_ERR_IO with zlib's message for a damaged file.  *out_n receives the inflated size; the first
 * min(cap, size) bytes are written, so a caller whose capacity was too small calls again.  g2s_test_last_reads_gzip
 * tells the call's windows, chunks and starts afterwards. */
int g2s_test_gzip_inflate(const void* bytes, size_t n, int device, uint32_t chunk_bytes, uint32_t window_chunks, uint8_t* out,
                          size_t cap, size_t* out_n, int* outcome);

/* TEST HOOK: the chunked device inflate (csrc/gzip_inflate.h) in the process's last g2s_graph_build_files,
 * g2s_test_reads_text or g2s_test_gzip_inflate.  files: the gzip files the route was tried on; windows; chunks: the
 * chunks those windows covered; starts_found: the block starts the finder gave; absorbed: the chunks decoded by the chunk
 * in front of them; members: the gzip members of the files the route completed; outcome: the GzipOutcome of the last
 * file given back to zlib (0: none was); peak_device_bytes: the largest window footprint asked of the allocator.  All 0
 * when the mode was not asked for.  Any pointer may be NULL. */
int g2s_test_last_reads_gzip(uint64_t* files, uint64_t* windows, uint64_t* chunks, uint64_t* starts_found, uint64_t* absorbed,
                             uint64_t* members, int* outcome, uint64_t* peak_device_bytes);

#ifdef __cplusplus
}
#endif
#endif /* G2S_TEST_H_ */
