"""ctypes binding of include/g2s.h (the drop-in boundary for
/root/reference/src/Gap2Seq.cpp:858 ``Gap2Seq::fill_gap`` and its caller
``Gap2Seq::execute`` :161-438).  Names follow the C ABI one to one.

No compute lives here.  If ``libg2s_hip.so`` is missing the import of the library
raises; if no gfx950 device is usable every fill call raises G2SError
(G2S_ERR_NO_DEVICE) — there is no CPU path to fall back to.
"""
import ctypes as C
import os

G2S_OK = 0
G2S_ERR_IO = -2
G2S_ERR_NO_DEVICE = -3
G2S_ERR_STATE = -6
G2S_INVALID_NODE = 0xFFFFFFFF
G2S_MAX_PATHS = 2147483647 // 2 - 1
G2S_MAX_IN_FLIGHT = 3  # include/g2s.h: lists begun and not ended on one session
G2S_GROUP_PER_SESSION = (1 << 64) - 1  # include/g2s.h: g2s_session_set_team cuts every long list into one group per session
G2S_GAP_SKIPPED = 0x1
G2S_GAP_Q7 = 0x2
G2S_GAP_MEM_EXCEEDED = 0x4
G2S_GAP_BACKTRACE_FAIL = 0x8
G2S_GAP_BAD_FLANK = 0x10
G2S_GAP_PHASE_D = 0x20


class G2SError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("g2s error %d: %s" % (code, msg))
        self.code = code


class g2s_params(C.Structure):
    _fields_ = [("d_err", C.c_int32), ("skip_confident", C.c_int32), ("all_paths", C.c_int32),
                ("unique_paths", C.c_int32), ("max_mem", C.c_int64), ("randseed", C.c_uint32),
                ("host_threads", C.c_int32)]


class g2s_gap(C.Structure):
    _fields_ = [("left", C.c_char_p), ("right", C.c_char_p), ("left_len", C.c_int32), ("right_len", C.c_int32),
                ("gap_len", C.c_int32), ("lmf", C.c_int32), ("rmf", C.c_int32),
                ("skip_if_prev_right_fuz_gt", C.c_int32)]


class g2s_result(C.Structure):
    _fields_ = [("count", C.c_int32), ("left_fuz", C.c_int32), ("right_fuz", C.c_int32), ("flags", C.c_uint32),
                ("fill_off", C.c_uint64), ("fill_len", C.c_int32), ("draws", C.c_int32),
                ("vertices", C.c_uint64), ("edges", C.c_uint64), ("nontrivial_components", C.c_uint64),
                ("size_nontrivial_components", C.c_uint64), ("vertices_final", C.c_uint64),
                ("edges_final", C.c_uint64), ("phaseC_count", C.c_int32), ("n_lengths", C.c_int32),
                ("lengths", C.c_int32 * 2), ("backtrace_depth", C.c_int32), ("backtrace_final_d", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class g2s_timing(C.Structure):
    _fields_ = [("ms_right_bfs", C.c_double), ("ms_left_dp", C.c_double), ("ms_extract", C.c_double),
                ("ms_d2h", C.c_double), ("ms_host_post", C.c_double), ("ms_total", C.c_double),
                ("xA", C.c_uint64), ("sA", C.c_uint64), ("xB", C.c_uint64), ("sB", C.c_uint64),
                ("xD", C.c_uint64), ("sD", C.c_uint64), ("flank_bytes", C.c_uint64), ("fill_bytes", C.c_uint64),
                ("launches_left_dp", C.c_uint32), ("retried_gaps", C.c_uint32),
                # (the eight fields from ms_fill_lds to rs_pool_gaps: a retired tier, kept for the layout, always zero)
                ("ms_fill_lds", C.c_double), ("ms_extract_lds", C.c_double), ("x_fill_lds", C.c_uint64),
                ("s_fill_lds", C.c_uint64), ("lds_tier_gaps", C.c_uint32), ("lds_launches", C.c_uint32),
                ("log_pool_gaps", C.c_uint32), ("rs_pool_gaps", C.c_uint32), ("ms_prepare", C.c_double),
                ("ms_fill_seg", C.c_double), ("seg_tier_gaps", C.c_uint32), ("seg_launches", C.c_uint32),
                ("seg_segments", C.c_uint64), ("ms_fill_segx", C.c_double), ("segx_tier_gaps", C.c_uint32),
                ("segx_launches", C.c_uint32), ("watchdog_gaps", C.c_uint32), ("seg2_launches", C.c_uint32),
                ("ms_d3", C.c_double), ("resident_launches", C.c_uint32), ("resident_fallbacks", C.c_uint32),
                ("draw_dependent_gaps", C.c_uint64), ("d3_table_entries", C.c_uint64),
                ("host_finished_gaps", C.c_uint32), ("team_groups", C.c_uint32), ("team_sessions", C.c_uint32),
                ("team_groups_by_session", C.c_uint32 * 16), ("seg_timed_launches", C.c_uint32), ("team_d3_sharded", C.c_uint32), ("traced_in_fill_gaps", C.c_uint32),
                ("team_ms_fill", C.c_double * 16), ("team_ms_d3", C.c_double * 16), ("team_ms_wall", C.c_double * 16),
                ("host_us", C.c_double * 8), ("guessed_in_fill_gaps", C.c_uint32), ("guessed_groups", C.c_uint32),
                ("guessed_groups_resent", C.c_uint32), ("reserved1", C.c_uint32)]


class g2s_run_opts(C.Structure):
    _fields_ = [("k", C.c_int32), ("solid", C.c_int32), ("max_fuz", C.c_int32), ("nb_cores", C.c_int32),
                ("max_mem_gb", C.c_double)]


class g2s_filter_opts(C.Structure):
    _fields_ = [("mean_insert", C.c_int32), ("std_dev", C.c_int32), ("breakpoint", C.c_int32), ("gap_length", C.c_int32),
                ("flank_length", C.c_int32), ("unmapped_only", C.c_int32), ("threads", C.c_int32),
                ("scaffold", C.c_char_p)]


class g2s_filter_gap(C.Structure):
    _fields_ = [("scaffold", C.c_char_p), ("breakpoint", C.c_int32), ("gap_length", C.c_int32),
                ("flank_length", C.c_int32)]


class g2s_filter_stats(C.Structure):
    _fields_ = [("file_passes", C.c_uint32), ("on_device", C.c_uint32), ("ms_inflate", C.c_double),
                ("ms_join", C.c_double), ("ms_text", C.c_double)]


class g2s_read_pool(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("bases", C.POINTER(C.c_char)), ("base_off", C.POINTER(C.c_uint64)),
                ("names", C.POINTER(C.c_char)), ("name_off", C.POINTER(C.c_uint64)), ("gap_begin", C.POINTER(C.c_uint64)),
                ("gap_read", C.POINTER(C.c_uint32)), ("n_unmapped", C.c_uint64), ("unmapped_read", C.POINTER(C.c_uint32))]


# every symbol include/g2s.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
TEXT_FN = C.CFUNCTYPE(None, C.POINTER(C.c_char), C.c_size_t, C.c_void_p)  # g2s_text_fn
_SIGS = {
    "g2s_abi_version": (C.c_int, []),
    "g2s_fill_begin": (C.c_int, [_VP, C.POINTER(g2s_gap), C.c_size_t, C.POINTER(g2s_result), C.c_void_p, C.c_size_t]),
    "g2s_fill_end": (C.c_int, [_VP]),
    "g2s_fill_in_flight": (C.c_int, [_VP]),
    "g2s_fill_in_flight_launched": (C.c_int, [_VP]),
    "g2s_share_begin": (C.c_int, [_VP, C.POINTER(g2s_gap), C.c_size_t, C.POINTER(g2s_result), C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_uint64)]),
    "g2s_share_tables": (C.c_int, [_VP, C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(C.c_uint32))]),
    "g2s_share_trace": (C.c_int, [_VP, C.c_uint32]),
    "g2s_share_end": (C.c_int, [_VP, C.c_uint64]),
    "g2s_backtrace_text": (C.c_size_t, [C.POINTER(g2s_gap), C.POINTER(g2s_result), C.c_int, C.c_char_p, C.c_size_t]),
    "g2s_last_error": (C.c_char_p, []),
    "g2s_graph_build_files": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "g2s_graph_build_seqs": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.POINTER(_VP)]),
    "g2s_graph_build_sets": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int,
                                       C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "g2s_graph_build_pool": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8),
                                       C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "g2s_graph_build_pool_reach": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8),
                                             C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(g2s_gap), C.POINTER(C.c_int32),
                                             C.POINTER(_VP)]),
    "g2s_graph_build_seqs_reach": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(g2s_gap), C.POINTER(C.c_int32), C.c_uint64, C.c_int, C.POINTER(_VP)]),
    "g2s_graph_build_files_reach": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(g2s_gap), C.POINTER(C.c_int32),
                                              C.c_uint64, C.c_int, C.POINTER(_VP)]),
    "g2s_scaffolds_reach": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "g2s_reach_records_count": (C.c_uint64, [_VP]),
    "g2s_reach_records_gaps": (C.POINTER(g2s_gap), [_VP]),
    "g2s_reach_records_radii": (C.POINTER(C.c_int32), [_VP]),
    "g2s_reach_records_free": (None, [_VP]),
    "g2s_graph_bounded": (C.c_int, [_VP]),
    "g2s_test_last_graph_reach": (C.c_int, [C.POINTER(C.c_uint64)] * 5 + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_int),
                                                                                                                  C.POINTER(C.c_double)]),
    "g2s_test_last_pool_reach": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "g2s_test_last_pool_build": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_int)]),
    "g2s_test_last_solid_count": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "g2s_test_plan_passes": (C.c_int, [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "g2s_test_seg_back_record": (C.c_int, [_VP, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]),
    "g2s_graph_num_sets": (C.c_uint32, [_VP]),
    "g2s_graph_set_nodes": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "g2s_graph_set_node": (C.c_uint32, [_VP, C.c_uint32, C.c_char_p]),
    "g2s_graph_save": (C.c_int, [_VP, C.c_char_p]),
    "g2s_graph_load": (C.c_int, [C.c_char_p, C.POINTER(_VP)]),
    "g2s_graph_free": (None, [_VP]),
    "g2s_graph_k": (C.c_int, [_VP]),
    "g2s_graph_solid": (C.c_int, [_VP]),
    "g2s_graph_num_kmers": (C.c_uint64, [_VP]),
    "g2s_graph_num_unitigs": (C.c_uint64, [_VP]),
    "g2s_graph_node": (C.c_uint32, [_VP, C.c_char_p]),
    "g2s_graph_successors": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint32)]),
    "g2s_graph_predecessors": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint32)]),
    "g2s_graph_node_string": (C.c_int, [_VP, C.c_uint32, C.c_char_p]),
    "g2s_graph_upload": (C.c_int, [_VP, C.c_int]),
    "g2s_graph_device_bytes": (C.c_uint64, [_VP, C.c_int]),
    "g2s_session_create": (C.c_int, [_VP, C.c_int, C.POINTER(g2s_params), C.POINTER(_VP)]),
    "g2s_session_destroy": (None, [_VP]),
    "g2s_session_srand": (C.c_int, [_VP, C.c_uint32]),
    "g2s_session_skip_draws": (C.c_int, [_VP, C.c_uint64]),
    "g2s_session_graph": (_VP, [_VP]),
    "g2s_session_get_params": (C.c_int, [_VP, C.POINTER(g2s_params)]),
    "g2s_batch_prepare": (C.c_int, [_VP, C.POINTER(g2s_gap), C.c_size_t, C.POINTER(_VP)]),
    "g2s_batch_run": (C.c_int, [_VP, C.POINTER(g2s_result), C.c_char_p, C.c_size_t]),
    "g2s_batch_arena_bytes": (C.c_size_t, [_VP]),
    "g2s_batch_timing": (C.c_int, [_VP, C.POINTER(g2s_timing)]),
    "g2s_batch_free": (None, [_VP]),
    "g2s_session_last_timing": (C.c_int, [_VP, C.POINTER(g2s_timing)]),
    "g2s_fill_batch": (C.c_int, [_VP, C.POINTER(g2s_gap), C.c_size_t, C.POINTER(g2s_result), C.c_char_p,
                                 C.c_size_t]),
    "g2s_team_fill": (C.c_int, [C.POINTER(_VP), C.c_int, C.POINTER(g2s_gap), C.c_size_t, C.c_size_t,
                                C.POINTER(g2s_result), C.c_char_p, C.c_size_t, C.POINTER(g2s_timing)]),
    "g2s_team_arena_bytes": (C.c_size_t, [_VP, C.POINTER(g2s_gap), C.c_size_t]),
    "g2s_fill_sets": (C.c_int, [_VP, C.POINTER(g2s_gap), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(g2s_result),
                                C.c_char_p, C.c_size_t]),
    "g2s_session_set_team": (C.c_int, [_VP, C.POINTER(_VP), C.c_int, C.c_size_t]),
    "g2s_execute_scaffolds_stream": (C.c_int, [_VP, C.POINTER(g2s_run_opts), C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t,
                                             TEXT_FN, TEXT_FN, _VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "g2s_execute_scaffolds": (C.c_int, [_VP, C.POINTER(g2s_run_opts), C.c_char_p, C.c_char_p, C.c_char_p,
                                        C.POINTER(_VP), C.POINTER(_VP), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "g2s_execute_single": (C.c_int, [_VP, C.POINTER(g2s_run_opts), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                     C.c_int32, C.POINTER(_VP), C.POINTER(_VP)]),
    "g2s_free": (None, [_VP]),
    "g2s_host_alloc": (_VP, [C.c_size_t]),
    "g2s_host_free": (None, [_VP]),
    "g2s_cut_scaffolds": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                    C.c_char_p, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]),
    "g2s_merge_scaffolds": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(_VP),
                                      C.POINTER(_VP)]),
    "g2s_filter_reads": (C.c_int, [C.c_char_p, C.POINTER(g2s_filter_opts), C.POINTER(_VP), C.POINTER(_VP),
                                   C.POINTER(_VP), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "g2s_filter_reads_mem": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(g2s_filter_opts), C.POINTER(_VP),
                                       C.POINTER(_VP), C.POINTER(_VP), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "g2s_filter_reads_gaps": (C.c_int, [C.c_char_p, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap), C.c_size_t,
                                        C.c_int, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64), C.POINTER(_VP), C.POINTER(C.c_int64),
                                        C.POINTER(g2s_filter_stats)]),
    "g2s_filter_reads_gaps_mem": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap),
                                            C.c_size_t, C.c_int, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_VP),
                                            C.POINTER(C.c_int64), C.POINTER(g2s_filter_stats)]),
    "g2s_filter_reads_gaps_pool": (C.c_int, [C.c_char_p, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap), C.c_size_t,
                                             C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(g2s_read_pool)),
                                             C.POINTER(C.c_int64), C.POINTER(g2s_filter_stats)]),
    "g2s_filter_reads_gaps_pool_mem": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap),
                                                 C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(g2s_read_pool)),
                                                 C.POINTER(C.c_int64), C.POINTER(g2s_filter_stats)]),
    "g2s_read_pool_free": (None, [C.POINTER(g2s_read_pool)]),
    "g2s_filter_reads_gaps_dpool": (C.c_int, [C.c_char_p, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap), C.c_size_t,
                                              C.c_int, C.c_int, C.POINTER(_VP), C.POINTER(C.c_int64),
                                              C.POINTER(g2s_filter_stats)]),
    "g2s_filter_reads_gaps_dpool_mem": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(g2s_filter_opts), C.POINTER(g2s_filter_gap),
                                                  C.c_size_t, C.c_int, C.c_int, C.POINTER(_VP), C.POINTER(C.c_int64),
                                                  C.POINTER(g2s_filter_stats)]),
    "g2s_device_pool_view": (C.POINTER(g2s_read_pool), [_VP]),
    "g2s_device_pool_device": (C.c_int, [_VP]),
    "g2s_device_pool_bytes": (C.c_uint64, [_VP]),
    "g2s_device_pool_read": (C.c_int, [_VP, C.c_uint64, C.c_char_p]),
    "g2s_device_pool_free": (None, [_VP]),
    "g2s_graph_build_dpool_reach": (C.c_int, [C.POINTER(_VP), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8), C.c_uint32, C.c_int,
                                              C.c_int, C.c_int, C.POINTER(g2s_gap), C.POINTER(C.c_int32), C.POINTER(_VP)]),
    "g2s_test_last_dpool": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]),
    "g2s_filter_last_error": (C.c_char_p, []),
    "g2s_device_count": (C.c_int, []),
    "g2s_synth_genome": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(_VP)]),
    "g2s_synth_gaps": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                 C.POINTER(_VP)]),
    "g2s_test_rand_skip": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_int32)]),
    "g2s_test_rand_stream": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "g2s_test_device_rand": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_int32)]),
    "g2s_test_d3_tables": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                     C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]),
    "g2s_test_d3_chain_launches": (C.c_uint64, []),
    "g2s_test_post_closure": (C.c_int, [_VP, C.POINTER(g2s_params), C.POINTER(g2s_gap), C.c_uint32,
                                        C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64), C.c_int32, C.c_int32,
                                        C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint32, C.c_uint64,
                                        C.POINTER(g2s_result), C.c_char_p]),
    "g2s_test_graph_tables": (C.c_int, [_VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "g2s_test_post_segments": (C.c_int, [_VP, C.POINTER(g2s_params), C.POINTER(g2s_gap), C.c_uint32,
                                         C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                         C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(g2s_result), C.c_char_p,
                                         C.POINTER(C.c_int32)]),
    "g2s_test_seg_expand": (C.c_int, [_VP, C.POINTER(g2s_params), C.POINTER(g2s_gap), C.c_uint32, C.POINTER(C.c_uint32),
                                      C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.c_uint32, C.POINTER(C.c_uint64)]),
    "g2s_test_worker_pool": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "g2s_test_group_queue": (C.c_int, [C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(C.c_int32)]),
    "g2s_test_group_queue_slow": (C.c_int, [C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]),
    "g2s_test_filter_join": (C.c_int, [C.c_int, C.c_int32, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                                       C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64)]),
    "g2s_test_reads_text": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "g2s_test_last_reads_load": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.c_uint64, C.POINTER(C.c_uint64)]),
    "g2s_test_last_reads_bam": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "g2s_test_last_reads_bam_stream": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "g2s_test_bgzf_inflate": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint8), C.c_size_t,
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "g2s_test_last_filter_inflate": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "g2s_test_bam_rows": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t, C.c_uint64, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "g2s_test_bam_rows_kept": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t, C.c_uint64, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "g2s_test_name_hash": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "g2s_test_last_filter_rows": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "g2s_filter_set_one_pass": (C.c_int, [C.c_int]),
    "g2s_reads_set_device_gzip": (C.c_int, [C.c_int]),
    "g2s_test_gzip_inflate": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8),
                                        C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "g2s_test_last_reads_gzip": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "g2s_test_last_filter_text": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "g2s_test_bam_text": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.c_uint64, C.c_int, C.c_int,
                                    C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_uint64,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64,
                                    C.POINTER(C.c_uint64)]),
    "g2s_test_bam_text_store": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint64, C.c_int,
                                          C.c_int, C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                                          C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.c_uint64, C.POINTER(C.c_uint64)]),
    "g2s_test_filter_store_plan": (C.c_int, [C.c_char_p, C.c_size_t] + [C.POINTER(C.c_uint64)] * 6),
    "g2s_test_bam_store": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_uint8), C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64)]),
    "g2s_test_last_filter_store": (C.c_int, [C.POINTER(C.c_int)] + [C.POINTER(C.c_uint64)] * 5 + [C.POINTER(C.c_int)]),
    "g2s_graph_validate": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "g2s_test_post_gap": (C.c_int, [_VP, C.POINTER(g2s_params), C.POINTER(g2s_gap), C.c_int32,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int32,
                                    C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                                    C.POINTER(g2s_result), C.c_char_p]),
}


def library_path():
    # (G2S_LIBRARY: an instrumented build of the same sources, tools/ only — the product library stays where it is)
    return os.environ.get("G2S_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2s_hip.so")


_LIB = None


def load_library():
    """Load the in-tree HIP extension; raises OSError when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc, gfx950). There is no CPU fallback." % path)
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)  # AttributeError = ABI symbol missing
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _check(rc):
    if rc != G2S_OK:
        raise G2SError(rc, (load_library().g2s_last_error() or b"").decode("utf-8", "replace"))


def _take_text(ptr):
    lib = load_library()
    if not ptr:
        return ""
    s = C.string_at(ptr).decode("ascii")
    lib.g2s_free(ptr)
    return s


class G2S:
    """Namespace for the free functions of the ABI."""

    @staticmethod
    def device_count():
        return load_library().g2s_device_count()

    @staticmethod
    def synth_genome(length, variant, seed):
        out = _VP()
        _check(load_library().g2s_synth_genome(length, variant, seed, C.byref(out)))
        return _take_text(out)

    @staticmethod
    def synth_gaps(reads_fasta, k, fuz, ngaps, min_len, max_len, seed):
        out = _VP()
        _check(load_library().g2s_synth_gaps(reads_fasta.encode("ascii"), k, fuz, ngaps, min_len, max_len, seed,
                                             C.byref(out)))
        return _take_text(out)


def cut_scaffolds(scaffolds_text, k=31, fuz=10, mask=False, no_split=False, labels=("scaffolds.fa", "contigs.fa", "gaps.fa", "gaps.bed")):
    """g2s_cut_scaffolds (GapCutter): returns (contigs_fasta, gaps_fasta, bed, log)."""
    outs = [_VP(), _VP(), _VP(), _VP()]
    _check(load_library().g2s_cut_scaffolds(scaffolds_text.encode("ascii"), k, fuz, int(mask), int(no_split),
                                            *[x.encode() for x in labels], *[C.byref(o) for o in outs]))
    return tuple(_take_text(o) for o in outs)


def merge_scaffolds(contigs_text, gaps_text, labels=("merged.fa", "contigs.fa", "filled.fa")):
    """g2s_merge_scaffolds (GapMerger): returns (scaffolds_fasta, log)."""
    out, log = _VP(), _VP()
    _check(load_library().g2s_merge_scaffolds(contigs_text.encode("ascii"), gaps_text.encode("ascii"),
                                              *[x.encode() for x in labels], C.byref(out), C.byref(log)))
    return _take_text(out), _take_text(log)


def filter_reads(bam, mean, std_dev, scaffold, breakpoint, gap_length=-1, flank_length=-1, unmapped_only=False,
                 threads=0):
    """g2s_filter_reads / g2s_filter_reads_mem (ReadFilter): `bam` is a path (str) or the file's bytes.
    Returns (fasta, stdout_text, stderr_text, extracted, total)."""
    lib = load_library()
    o = g2s_filter_opts(mean, std_dev, breakpoint, gap_length, flank_length, int(unmapped_only), threads,
                        scaffold.encode())
    outs = [_VP(), _VP(), _VP()]
    ext, tot = C.c_int64(0), C.c_int64(0)
    tail = [C.byref(o)] + [C.byref(x) for x in outs] + [C.byref(ext), C.byref(tot)]
    if isinstance(bam, (bytes, bytearray)):
        rc = lib.g2s_filter_reads_mem(bytes(bam), len(bam), *tail)
    else:
        rc = lib.g2s_filter_reads(str(bam).encode(), *tail)
    if rc != G2S_OK:
        raise G2SError(rc, (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace"))
    texts = []
    for x in outs:  # (read names are bytes of the BAM file: not necessarily ASCII)
        texts.append(C.string_at(x).decode("latin-1") if x else "")
        lib.g2s_free(x)
    return tuple(texts) + (ext.value, tot.value)


def filter_reads_gaps(bam, mean, std_dev, gaps, device=0, threads=0, unmapped=False):
    """g2s_filter_reads_gaps / g2s_filter_reads_gaps_mem: the reads of every gap of `gaps` from one library in two
    passes over the file.  `gaps`: (scaffold, breakpoint[, gap_length[, flank_length]]) tuples or dicts with those
    keys (gap_length and flank_length default to -1, as in filter_reads).  device -1 = the joins on host threads.
    Returns (per-gap list of (fasta, stdout_text, stderr_text, extracted, total) as filter_reads returns them, stats
    dict); with unmapped=True a third item, filter_reads(..., unmapped_only=True)'s tuple, from the same passes."""
    lib = load_library()
    arr = _filter_gap_array(gaps)
    n = len(gaps)
    o = g2s_filter_opts(mean, std_dev, 0, -1, -1, 0, threads, b"")
    fa, lg, wn = (_VP * max(1, n))(), (_VP * max(1, n))(), (_VP * max(1, n))()
    ext = (C.c_int64 * max(1, n))()
    tot, un_ext = C.c_int64(0), C.c_int64(0)
    un = _VP()
    st = g2s_filter_stats()
    tail = [C.byref(o), arr, n, device, fa, lg, wn, ext, C.byref(tot), C.byref(un) if unmapped else None,
            C.byref(un_ext), C.byref(st)]
    if isinstance(bam, (bytes, bytearray)):
        rc = lib.g2s_filter_reads_gaps_mem(bytes(bam), len(bam), *tail)
    else:
        rc = lib.g2s_filter_reads_gaps(str(bam).encode(), *tail)
    if rc != G2S_OK:
        raise G2SError(rc, (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace"))

    def take(p):  # (read names are bytes of the BAM file: not necessarily ASCII)
        s = C.string_at(p).decode("latin-1") if p else ""
        lib.g2s_free(p)
        return s
    out = [(take(fa[i]), take(lg[i]), take(wn[i]), ext[i], tot.value) for i in range(n)]
    stats = dict(file_passes=st.file_passes, on_device=st.on_device, ms_inflate=st.ms_inflate, ms_join=st.ms_join,
                 ms_text=st.ms_text)
    if not unmapped:
        return out, stats
    un_fa = take(un)
    un_log = "Extracted %d out of %d reads\n" % (un_ext.value, tot.value)
    return out, stats, (un_fa, un_log, "", un_ext.value, tot.value)


def _filter_gap_array(gaps):
    arr = (g2s_filter_gap * max(1, len(gaps)))()
    for i, g in enumerate(gaps):
        if isinstance(g, dict):
            g = (g["scaffold"], g["breakpoint"], g.get("gap_length", -1), g.get("flank_length", -1))
        g = tuple(g) + (-1,) * (4 - len(g))
        arr[i] = g2s_filter_gap(g[0].encode(), g[1], g[2], g[3])
    return arr


class ReadPool:
    """g2s_read_pool: every read some gap selected (or that is unmapped) held once, and every gap a list of indices
    into the pool.  seqs / names: the reads' bases / "name/1" or "name/2" as bytes (names None unless asked for);
    gap_reads(i): gap i's read indices in the order of filter_reads_gaps' FASTA; unmapped: the unmapped reads' indices;
    total: records in the file; stats: as filter_reads_gaps returns them."""

    def __init__(self, ptr, n_gaps, total, stats):
        self.p, self.n_gaps, self.total, self.stats = ptr, n_gaps, total, stats
        self._seqs = self._names = None

    def _take(self, text, off):
        p = self.p.contents
        n = p.n_reads
        raw = C.string_at(text, off[n]) if off[n] else b""
        return [raw[off[i]:off[i + 1]] for i in range(n)]

    @property
    def n_reads(self):
        return self.p.contents.n_reads

    @property
    def seqs(self):
        if self._seqs is None:
            self._seqs = self._take(self.p.contents.bases, self.p.contents.base_off)
        return self._seqs

    @property
    def names(self):
        if self._names is None and self.p.contents.names:
            self._names = self._take(self.p.contents.names, self.p.contents.name_off)
        return self._names

    def gap_reads(self, i):
        if not 0 <= i < self.n_gaps:
            raise IndexError(i)
        p = self.p.contents
        return p.gap_read[p.gap_begin[i]:p.gap_begin[i + 1]]

    @property
    def unmapped(self):
        p = self.p.contents
        return p.unmapped_read[0:p.n_unmapped]

    def _fasta(self, reads):  # (read names are bytes of the BAM file: not necessarily ASCII)
        if self.names is None:
            raise ValueError("the pool was made without names")
        return b"".join(b">" + self.names[r] + b"\n" + self.seqs[r] + b"\n" for r in reads).decode("latin-1")

    def fasta(self, i):
        """gap i's FASTA text: filter_reads_gaps' for that gap, byte for byte"""
        return self._fasta(self.gap_reads(i))

    def unmapped_fasta(self):
        return self._fasta(self.unmapped)

    @property
    def nbytes(self):
        """bytes of the arrays the pool holds"""
        p = self.p.contents
        n = p.n_reads
        b = p.base_off[n] + 8 * (n + 1) + 8 * (self.n_gaps + 1) + 4 * p.gap_begin[self.n_gaps] + 4 * p.n_unmapped
        if p.names:
            b += p.name_off[n] + 8 * (n + 1)
        return b

    def free(self):
        if self.p:
            load_library().g2s_read_pool_free(self.p)
            self.p = None


def filter_reads_gaps_pool(bam, mean, std_dev, gaps, device=0, threads=0, names=True, unmapped=True):
    """g2s_filter_reads_gaps_pool / _mem: filter_reads_gaps with the reads handed over as a ReadPool (every read held
    once however many gaps select it) instead of per-gap FASTA text.  `bam`, `gaps`, `device` as there."""
    lib = load_library()
    arr = _filter_gap_array(gaps)
    n = len(gaps)
    o = g2s_filter_opts(mean, std_dev, 0, -1, -1, 0, threads, b"")
    out = C.POINTER(g2s_read_pool)()
    tot = C.c_int64(0)
    st = g2s_filter_stats()
    tail = [C.byref(o), arr, n, device, int(bool(names)), int(bool(unmapped)), C.byref(out), C.byref(tot), C.byref(st)]
    if isinstance(bam, (bytes, bytearray)):
        rc = lib.g2s_filter_reads_gaps_pool_mem(bytes(bam), len(bam), *tail)
    else:
        rc = lib.g2s_filter_reads_gaps_pool(str(bam).encode(), *tail)
    if rc != G2S_OK:
        raise G2SError(rc, (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace"))
    stats = dict(file_passes=st.file_passes, on_device=st.on_device, ms_inflate=st.ms_inflate, ms_join=st.ms_join,
                 ms_text=st.ms_text)
    return ReadPool(out, n, tot.value, stats)


class DevicePool:
    """g2s_device_pool: a ReadPool whose bases stay where the read filter made them — in device memory when one of the
    one-pass routes ran (`device` >= 0), in host memory otherwise (`device` -1).  The view's arrays as numpy arrays:
    base_off, name_off (the names themselves are never kept), gap_begin, gap_read, unmapped_read; n_reads; device_bytes;
    read(r): read r's bases (a copy from the device a call: for tests); total, stats as filter_reads_gaps returns them."""

    def __init__(self, handle, n_gaps, total, stats):
        import numpy as np
        self.h, self.n_gaps, self.total, self.stats = handle, n_gaps, total, stats
        v = load_library().g2s_device_pool_view(handle).contents
        self.n_reads = int(v.n_reads)

        def arr(ptr, n, dtype):
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)
        self.base_off = arr(v.base_off, self.n_reads + 1, np.uint64)
        self.name_off = arr(v.name_off, self.n_reads + 1, np.uint64)
        self.gap_begin = arr(v.gap_begin, n_gaps + 1, np.uint64)
        self.gap_read = arr(v.gap_read, int(self.gap_begin[n_gaps]), np.uint32)
        self.unmapped_read = arr(v.unmapped_read, int(v.n_unmapped), np.uint32)
        self.bases_is_null, self.names_is_null = not v.bases, not v.names

    @property
    def device(self):
        return load_library().g2s_device_pool_device(self.h)

    @property
    def device_bytes(self):
        return load_library().g2s_device_pool_bytes(self.h)

    def read(self, r):
        if not 0 <= r < self.n_reads:
            raise IndexError(r)
        n = int(self.base_off[r + 1] - self.base_off[r])
        buf = C.create_string_buffer(max(1, n))
        rc = load_library().g2s_device_pool_read(self.h, r, buf)
        if rc != G2S_OK:
            raise G2SError(rc, (load_library().g2s_filter_last_error() or b"").decode("utf-8", "replace"))
        return buf.raw[:n]

    def gap_reads(self, i):
        if not 0 <= i < self.n_gaps:
            raise IndexError(i)
        return [int(x) for x in self.gap_read[int(self.gap_begin[i]):int(self.gap_begin[i + 1])]]

    def free(self):
        if self.h:
            load_library().g2s_device_pool_free(self.h)
            self.h = None


def filter_reads_gaps_dpool(bam, mean, std_dev, gaps, device=0, threads=0, unmapped=True):
    """g2s_filter_reads_gaps_dpool / _mem: filter_reads_gaps_pool(names=True) handing over a DevicePool.  The call asks
    for one-pass mode by itself; filter_set_one_pass(0) forbids it and gives a host-held pool."""
    lib = load_library()
    arr = _filter_gap_array(gaps)
    n = len(gaps)
    o = g2s_filter_opts(mean, std_dev, 0, -1, -1, 0, threads, b"")
    out = _VP()
    tot = C.c_int64(0)
    st = g2s_filter_stats()
    tail = [C.byref(o), arr, n, device, int(bool(unmapped)), C.byref(out), C.byref(tot), C.byref(st)]
    if isinstance(bam, (bytes, bytearray)):
        rc = lib.g2s_filter_reads_gaps_dpool_mem(bytes(bam), len(bam), *tail)
    else:
        rc = lib.g2s_filter_reads_gaps_dpool(str(bam).encode(), *tail)
    if rc != G2S_OK:
        raise G2SError(rc, (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace"))
    stats = dict(file_passes=st.file_passes, on_device=st.on_device, ms_inflate=st.ms_inflate, ms_join=st.ms_join,
                 ms_text=st.ms_text)
    return DevicePool(out, n, tot.value, stats)


def test_last_dpool():
    """g2s_test_last_dpool: of the last filter_reads_gaps_dpool, whether its pool is device-held and the bytes of bases
    that became host memory; of the last pooled build, the text positions gathered on the device / packed on the host."""
    held, down, gathered, packed = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(load_library().g2s_test_last_dpool(C.byref(held), C.byref(down), C.byref(gathered), C.byref(packed)))
    return dict(held_on_device=held.value, bases_bytes_to_host=down.value, text_bytes_gathered_on_device=gathered.value,
                text_bytes_packed_on_host=packed.value)


class Graph:
    """g2s_graph: replaces gatb Graph::create / Graph::load (Gap2Seq.cpp:193-219)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_seqs(cls, seqs, k, solid, nthreads=0, reach=None, reach_mode=None):
        """g2s_graph_build_seqs; with `reach` = [(Gap, radius), ...] g2s_graph_build_seqs_reach: the graph of the solid
        k-mers within `radius` steps of the flank k-mers the fill looks up for some record's Gap (reach_radius(gap, d_err)
        loses nothing of that fill).  reach_mode: REACH_ALWAYS (the default with records), REACH_NEVER, REACH_AUTO."""
        lib = load_library()
        enc = [s.encode("ascii") if isinstance(s, str) else s for s in seqs]
        arr = (C.c_char_p * len(enc))(*enc)
        lens = (C.c_uint64 * len(enc))(*[len(e) for e in enc])
        h = _VP()
        if reach is not None:
            gaps, radius, keep = _reach_arrays(reach)
            _check(lib.g2s_graph_build_seqs_reach(arr, lens, len(enc), k, solid, nthreads, gaps, radius, len(reach),
                                                  REACH_ALWAYS if reach_mode is None else reach_mode, C.byref(h)))
            del keep
            return cls(h)
        _check(lib.g2s_graph_build_seqs(arr, lens, len(enc), k, solid, nthreads, C.byref(h)))
        return cls(h)

    @property
    def bounded(self):
        """True for a graph that reach records bounded (it belongs to its gap list, not to its reads)."""
        return bool(load_library().g2s_graph_bounded(self.h))

    @classmethod
    def from_sets(cls, sets, k, solid, nthreads=0):
        """g2s_graph_build_sets: one graph per read set (`sets`: a list of lists of sequences), numbered set-major."""
        lib = load_library()
        enc, owner = [], []
        for si, seqs in enumerate(sets):
            for s in seqs:
                enc.append(s.encode("ascii") if isinstance(s, str) else s)
                owner.append(si)
        n = len(enc)
        arr = (C.c_char_p * max(1, n))(*enc)
        lens = (C.c_uint64 * max(1, n))(*[len(e) for e in enc])
        sets_of = (C.c_uint32 * max(1, n))(*owner)
        h = _VP()
        _check(lib.g2s_graph_build_sets(arr, lens, sets_of, n, len(sets), k, solid, nthreads, C.byref(h)))
        return cls(h)

    @classmethod
    def from_pool(cls, seqs, set_lists, k, solid, shared=None, set_shared=None, nthreads=0, reach=None):
        """g2s_graph_build_pool: the set graph of from_sets for sets given as lists of indices into one pool of
        sequences (`set_lists`: per set, indices into `seqs`; a sequence may be in many sets, and twice in one).
        `shared`: indices of a list that every set with a true `set_shared` entry holds behind its own.
        `reach` (g2s_graph_build_pool_reach): per set, None or (gap, radius) — the set keeps only the k-mers within
        `radius` steps of the flank k-mers the fill looks up for `gap` (a Gap); a negative radius keeps the whole set.
        reach_radius(gap, d_err) is the radius that loses nothing of a fill with that d_err."""
        lib = load_library()
        enc = [s.encode("ascii") if isinstance(s, str) else s for s in seqs]
        n = len(enc)
        arr = (C.c_char_p * max(1, n))(*enc)
        lens = (C.c_uint64 * max(1, n))(*[len(e) for e in enc])
        begin, flat = [0], []
        for lst in set_lists:
            flat.extend(lst)
            begin.append(len(flat))
        set_begin = (C.c_uint64 * len(begin))(*begin)
        set_seq = (C.c_uint32 * max(1, len(flat)))(*flat)
        shared = list(shared) if shared is not None else []
        sh = (C.c_uint32 * len(shared))(*shared) if shared else None
        flags = None
        if set_shared is not None:
            if len(set_shared) != len(set_lists):
                raise ValueError("set_shared needs one entry a set")
            flags = (C.c_uint8 * max(1, len(set_lists)))(*[1 if f else 0 for f in set_shared])
        h = _VP()
        if reach is not None:
            if len(reach) != len(set_lists):
                raise ValueError("reach needs one entry a set")
            blank = Gap("", "", 0, 0, 0)
            gaps, keep = _gap_array([r[0] if r is not None else blank for r in reach])
            radius = (C.c_int32 * max(1, len(reach)))(*[int(r[1]) if r is not None else -1 for r in reach])
            _check(lib.g2s_graph_build_pool_reach(arr, lens, n, set_begin, set_seq, sh, len(shared), flags, len(set_lists), k,
                                                  solid, nthreads, gaps, radius, C.byref(h)))
            del keep
            return cls(h)
        _check(lib.g2s_graph_build_pool(arr, lens, n, set_begin, set_seq, sh, len(shared), flags, len(set_lists), k, solid,
                                        nthreads, C.byref(h)))
        return cls(h)

    @classmethod
    def from_dpools(cls, pools, set_lists, k, solid, shared=None, set_shared=None, reach=None, nthreads=0):
        """g2s_graph_build_dpool_reach: from_pool over the reads of `pools` (DevicePool objects), read r of pools[p]
        having the index sum(n_reads of pools[:p]) + r; the other arguments as from_pool's."""
        lib = load_library()
        hs = (_VP * max(1, len(pools)))(*[p.h for p in pools])
        begin, flat = [0], []
        for lst in set_lists:
            flat.extend(lst)
            begin.append(len(flat))
        set_begin = (C.c_uint64 * len(begin))(*begin)
        set_seq = (C.c_uint32 * max(1, len(flat)))(*flat)
        shared = list(shared) if shared is not None else []
        sh = (C.c_uint32 * len(shared))(*shared) if shared else None
        flags = None
        if set_shared is not None:
            if len(set_shared) != len(set_lists):
                raise ValueError("set_shared needs one entry a set")
            flags = (C.c_uint8 * max(1, len(set_lists)))(*[1 if f else 0 for f in set_shared])
        gaps = radius = keep = None
        if reach is not None:
            if len(reach) != len(set_lists):
                raise ValueError("reach needs one entry a set")
            blank = Gap("", "", 0, 0, 0)
            gaps, keep = _gap_array([r[0] if r is not None else blank for r in reach])
            radius = (C.c_int32 * max(1, len(reach)))(*[int(r[1]) if r is not None else -1 for r in reach])
        h = _VP()
        _check(lib.g2s_graph_build_dpool_reach(hs, len(pools), set_begin, set_seq, sh, len(shared), flags, len(set_lists), k,
                                               solid, nthreads, gaps, radius, C.byref(h)))
        del keep
        return cls(h)

    @property
    def num_sets(self):
        return load_library().g2s_graph_num_sets(self.h)

    def set_nodes(self, s):
        """(first node index, number of k-mers) of read set s."""
        first, cnt = C.c_uint64(), C.c_uint64()
        _check(load_library().g2s_graph_set_nodes(self.h, s, C.byref(first), C.byref(cnt)))
        return first.value, cnt.value

    def set_node(self, s, kmer):
        return load_library().g2s_graph_set_node(self.h, s, kmer.encode("ascii"))

    @classmethod
    def from_files(cls, reads_csv, k, solid, nthreads=0, reach=None, reach_mode=None):
        """The graph of a comma-separated list of read files: FASTA or FASTQ (plain, gzip or BGZF) and BAM, in any
        mixture, each told by its bytes, never by its name.  A BAM file gives every record that is neither secondary
        nor supplementary, mapped or not, as the read was sequenced (include/g2s.h: g2s_graph_build_files).
        reach, reach_mode: as from_seqs' (g2s_graph_build_files_reach)."""
        h = _VP()
        if reach is not None:
            gaps, radius, keep = _reach_arrays(reach)
            _check(load_library().g2s_graph_build_files_reach(reads_csv.encode(), k, solid, nthreads, gaps, radius, len(reach),
                                                              REACH_ALWAYS if reach_mode is None else reach_mode, C.byref(h)))
            del keep
            return cls(h)
        _check(load_library().g2s_graph_build_files(reads_csv.encode(), k, solid, nthreads, C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path):
        h = _VP()
        _check(load_library().g2s_graph_load(path.encode(), C.byref(h)))
        return cls(h)

    def save(self, path):
        _check(load_library().g2s_graph_save(self.h, path.encode()))

    @property
    def k(self):
        return load_library().g2s_graph_k(self.h)

    @property
    def num_kmers(self):
        return load_library().g2s_graph_num_kmers(self.h)

    @property
    def num_unitigs(self):
        return load_library().g2s_graph_num_unitigs(self.h)

    def validate(self):
        """(violations, text): bitmap / successor table / last-base table consistency (test hook)."""
        buf = C.create_string_buffer(2048)
        n = load_library().g2s_graph_validate(self.h, buf, 2048)
        return n, buf.value.decode()

    def node(self, kmer):
        return load_library().g2s_graph_node(self.h, kmer.encode("ascii"))

    def node_string(self, v):
        buf = C.create_string_buffer(self.k + 1)
        _check(load_library().g2s_graph_node_string(self.h, v, buf))
        return buf.value.decode()

    def successors(self, v):
        out = (C.c_uint32 * 4)()
        n = load_library().g2s_graph_successors(self.h, v, out)
        return [out[i] for i in range(n)]

    def predecessors(self, v):
        out = (C.c_uint32 * 4)()
        n = load_library().g2s_graph_predecessors(self.h, v, out)
        return [out[i] for i in range(n)]

    def upload(self, device=0):
        _check(load_library().g2s_graph_upload(self.h, device))

    def device_bytes(self, device=0):
        return load_library().g2s_graph_device_bytes(self.h, device)

    def free(self):
        if self.h:
            load_library().g2s_graph_free(self.h)
            self.h = None


class Gap:
    """Arguments of one fill_gap call (Gap2Seq.cpp:380-383)."""

    def __init__(self, left, right, gap_len, lmf, rmf, skip_if_prev_right_fuz_gt=-1):
        self.left, self.right, self.gap_len, self.lmf, self.rmf = left, right, gap_len, lmf, rmf
        self.skip_dep = skip_if_prev_right_fuz_gt


def make_params(d_err=500, skip_confident=False, all_paths=True, unique_paths=False, max_mem=20 << 30, randseed=1,
                host_threads=0):
    return g2s_params(d_err, int(skip_confident), int(all_paths), int(unique_paths), max_mem, randseed, host_threads)


REACH_NEVER, REACH_ALWAYS, REACH_AUTO = 0, 1, 2  # g2s_graph_build_seqs_reach's mode


def _reach_arrays(reach):
    """[(Gap, radius), ...] as the two arrays of the reach calls (+ what keeps their strings alive)"""
    gaps, keep = _gap_array([r[0] for r in reach])
    radius = (C.c_int32 * max(1, len(reach)))(*[int(r[1]) for r in reach])
    return gaps, radius, keep


def scaffolds_reach(text, k, fuz, d_err):
    """g2s_scaffolds_reach: [(Gap, radius)], one record per N-run of every scaffold record of `text`, for
    execute_scaffolds with max_fuz = fuz on a session with d_err — what Graph.from_seqs / from_files take as `reach`.
    A record without usable flanks has a Gap the fill rejects (no seeds)."""
    lib = load_library()
    h = _VP()
    _check(lib.g2s_scaffolds_reach(text.encode("ascii"), k, fuz, d_err, C.byref(h)))
    try:
        n = lib.g2s_reach_records_count(h)
        gaps, radii = lib.g2s_reach_records_gaps(h), lib.g2s_reach_records_radii(h)
        out = []
        for i in range(n):
            g = gaps[i]
            left, right = (g.left or b"").decode("ascii"), (g.right or b"").decode("ascii")
            out.append((Gap(left, right, g.gap_len, g.lmf, g.rmf), radii[i]))
        return out
    finally:
        lib.g2s_reach_records_free(h)


def test_last_graph_reach():
    """g2s_test_last_graph_reach: dict(records, seeds, seeds_in_full, full_kmers, kept_kmers, levels, passes, regrowths,
    on_device, ms_search) of the last bounded single-graph build"""
    u = [C.c_uint64() for _ in range(5)]
    w = [C.c_uint32() for _ in range(3)]
    on, ms = C.c_int(), C.c_double()
    _check(load_library().g2s_test_last_graph_reach(*[C.byref(x) for x in u + w], C.byref(on), C.byref(ms)))
    names = ("records", "seeds", "seeds_in_full", "full_kmers", "kept_kmers", "levels", "passes", "regrowths")
    out = {name: x.value for name, x in zip(names, u + w)}
    out["on_device"] = on.value
    out["ms_search"] = ms.value
    return out


def _gap_array(gaps):
    keep = []
    arr = (g2s_gap * max(1, len(gaps)))()
    for i, g in enumerate(gaps):
        l, r = g.left.encode("ascii"), g.right.encode("ascii")
        keep.append((l, r))
        arr[i] = g2s_gap(l, r, len(l), len(r), g.gap_len, g.lmf, g.rmf, g.skip_dep)
    return arr, keep


class FillResult:
    """g2s_result with the fill text resolved."""

    def __init__(self, r, arena):
        for name, _ in g2s_result._fields_:
            if name not in ("lengths", "reserved"):
                setattr(self, name, getattr(r, name))
        self.lengths = [r.lengths[i] for i in range(r.n_lengths)]
        # (the reference's "Unable to backtrace!" line minus the k-mer, which g2s_backtrace_text reads from the gap)
        self.backtrace_msg = ("Unable to backtrace! %d %d" % (r.backtrace_depth, r.backtrace_final_d)) if r.flags & G2S_GAP_BACKTRACE_FAIL else ""
        self.fill = arena[r.fill_off:r.fill_off + r.fill_len].decode("ascii") if r.fill_len > 0 else ""
        self.substats = [r.vertices, r.edges, r.nontrivial_components, r.size_nontrivial_components,
                         r.vertices_final, r.edges_final]


class HostBuffer:
    """g2s_host_alloc: page-locked memory the kernels write directly (results, fill arena)."""

    def __init__(self, nbytes):
        self.nbytes = max(16, int(nbytes))
        self.p = load_library().g2s_host_alloc(self.nbytes)
        if not self.p:
            raise MemoryError("g2s_host_alloc(%d) failed" % self.nbytes)

    def array(self, ctype, count):
        return (ctype * count).from_address(self.p)

    @property
    def raw(self):
        return C.string_at(self.p, self.nbytes)

    def free(self):
        if self.p:
            load_library().g2s_host_free(self.p)
            self.p = None


class Session:
    """g2s_session: one GPU, one rand() stream."""

    def __init__(self, graph, device=0, **kw):
        self.graph = graph
        self.params = make_params(**kw)
        h = _VP()
        _check(load_library().g2s_session_create(graph.h, device, C.byref(self.params), C.byref(h)))
        self.h = h

    def last_timing(self):
        """g2s_session_last_timing: the g2s_timing of the last list this session finished."""
        t = g2s_timing()
        _check(load_library().g2s_session_last_timing(self.h, C.byref(t)))
        return t

    def srand(self, seed, skip=0):
        _check(load_library().g2s_session_srand(self.h, seed))
        if skip:
            _check(load_library().g2s_session_skip_draws(self.h, skip))

    def fill_batch(self, gaps, want_timing=False, pinned=False):
        """prepare + run; returns list of FillResult (and g2s_timing).  pinned: results and arena in
        g2s_host_alloc memory (the kernels then write them directly when the list is finished on the device)."""
        lib = load_library()
        arr, keep = _gap_array(gaps)
        b = _VP()
        _check(lib.g2s_batch_prepare(self.h, arr, len(gaps), C.byref(b)))
        bufs = []
        try:
            nbytes = lib.g2s_batch_arena_bytes(b)
            if pinned:
                bufs = [HostBuffer(max(1, nbytes)), HostBuffer(C.sizeof(g2s_result) * max(1, len(gaps)))]
                arena = bufs[0]
                res = bufs[1].array(g2s_result, max(1, len(gaps)))
                _check(lib.g2s_batch_run(b, res, C.cast(arena.p, C.c_char_p), nbytes))
            else:
                arena = C.create_string_buffer(max(1, nbytes))
                res = (g2s_result * max(1, len(gaps)))()
                _check(lib.g2s_batch_run(b, res, arena, nbytes))
            t = g2s_timing()
            _check(lib.g2s_batch_timing(b, C.byref(t)))
            raw = arena.raw
            out = [FillResult(res[i], raw) for i in range(len(gaps))]
        finally:
            lib.g2s_batch_free(b)
            for hb in bufs:
                hb.free()
        return (out, t) if want_timing else out

    def fill_lists_overlapped(self, lists, pinned=True, depth=G2S_MAX_IN_FLIGHT):
        """g2s_fill_begin / g2s_fill_end over consecutive lists, `depth` in flight: list i+depth-1 is begun before
        list i is ended.  Returns the lists' results in order (and the timing of the last list ended)."""
        lib = load_library()
        ctx = []
        for gaps in lists:
            arr, keep = _gap_array(gaps)
            nbytes = lib.g2s_team_arena_bytes(self.h, arr, len(gaps))
            if pinned:
                arena = HostBuffer(max(1, nbytes))
                rbuf = HostBuffer(C.sizeof(g2s_result) * max(1, len(gaps)))
                res = rbuf.array(g2s_result, max(1, len(gaps)))
                ctx.append(dict(arr=arr, keep=keep, n=len(gaps), nbytes=nbytes, arena=arena, rbuf=rbuf, res=res, ap=C.cast(arena.p, C.c_void_p)))
            else:
                arena = C.create_string_buffer(max(1, nbytes))
                res = (g2s_result * max(1, len(gaps)))()
                ctx.append(dict(arr=arr, keep=keep, n=len(gaps), nbytes=nbytes, arena=arena, rbuf=None, res=res, ap=C.cast(arena, C.c_void_p)))
        out = []
        t = g2s_timing()
        try:
            for i, c in enumerate(ctx):
                _check(lib.g2s_fill_begin(self.h, c["arr"], c["n"], c["res"], c["ap"], c["nbytes"]))
                if i >= depth - 1:
                    _check(lib.g2s_fill_end(self.h))
            while lib.g2s_fill_in_flight(self.h) > 0:
                _check(lib.g2s_fill_end(self.h))
            _check(lib.g2s_session_last_timing(self.h, C.byref(t)))
            for c in ctx:
                raw = c["arena"].raw
                out.append([FillResult(c["res"][i], raw) for i in range(c["n"])])
        finally:
            # (an error between begin and end: the lists still in flight write into these buffers — end them,
            # whatever they return, before the buffers go)
            while lib.g2s_fill_in_flight(self.h) > 0:
                lib.g2s_fill_end(self.h)
            for c in ctx:
                if c["rbuf"] is not None:
                    c["rbuf"].free()
                    c["arena"].free()
        return out, t

    def in_flight(self):
        """g2s_fill_in_flight: lists begun and not ended."""
        return load_library().g2s_fill_in_flight(self.h)

    def in_flight_launched(self):
        """g2s_fill_in_flight_launched: how many of the lists in flight have their fill kernels queued on the device(s)
        (a team's list: on every share's device)."""
        return load_library().g2s_fill_in_flight_launched(self.h)

    def fill_batch_onecall(self, gaps, pinned=False, want_timing=False):
        """g2s_fill_batch (prepare + run + free in one ABI call; lists longer than the group size
        go through the group pipeline, with the session's team when it has one)."""
        lib = load_library()
        arr, keep = _gap_array(gaps)
        nbytes = lib.g2s_team_arena_bytes(self.h, arr, len(gaps))
        bufs = []
        try:
            if pinned:
                bufs = [HostBuffer(max(1, nbytes)), HostBuffer(C.sizeof(g2s_result) * max(1, len(gaps)))]
                arena, res = bufs[0], bufs[1].array(g2s_result, max(1, len(gaps)))
                _check(lib.g2s_fill_batch(self.h, arr, len(gaps), res, C.cast(arena.p, C.c_char_p), nbytes))
            else:
                arena = C.create_string_buffer(max(1, nbytes))
                res = (g2s_result * max(1, len(gaps)))()
                _check(lib.g2s_fill_batch(self.h, arr, len(gaps), res, arena, nbytes))
            raw = arena.raw
            out = [FillResult(res[i], raw) for i in range(len(gaps))]
        finally:
            for hb in bufs:
                hb.free()
        if want_timing:
            t = g2s_timing()
            _check(lib.g2s_session_last_timing(self.h, C.byref(t)))
            return out, t
        return out

    def fill_sets(self, gaps, gap_set, want_timing=False):
        """g2s_fill_sets: gap i filled in read set gap_set[i] of a set graph, every gap from a fresh srand(randseed);
        returns what fill_batch returns.  Lists of 256 gaps or more are finished on the device (resident mode,
        G2S_RESIDENT=0|1 as for fill_batch); the timing sums the list's groups, resident_launches /
        resident_fallbacks / host_finished_gaps included."""
        lib = load_library()
        if len(gap_set) != len(gaps):
            raise ValueError("fill_sets: one set id per gap")
        arr, keep = _gap_array(gaps)
        ids = (C.c_uint32 * max(1, len(gaps)))(*gap_set)
        nbytes = lib.g2s_team_arena_bytes(self.h, arr, len(gaps))
        arena = C.create_string_buffer(max(1, nbytes))
        res = (g2s_result * max(1, len(gaps)))()
        _check(lib.g2s_fill_sets(self.h, arr, ids, len(gaps), res, arena, nbytes))
        raw = arena.raw
        out = [FillResult(res[i], raw) for i in range(len(gaps))]
        if want_timing:
            t = g2s_timing()
            _check(lib.g2s_session_last_timing(self.h, C.byref(t)))
            return out, t
        return out

    def set_team(self, helpers, group_size=0):
        """g2s_session_set_team: fill_batch / execute_* on this session use self + helpers."""
        arr = (_VP * max(1, len(helpers)))(*[h.h for h in helpers])
        _check(load_library().g2s_session_set_team(self.h, arr, len(helpers), group_size))
        self._helpers = list(helpers)

    def prepare(self, gaps):
        """g2s_batch_prepare; returns an opaque PreparedBatch to run repeatedly."""
        return PreparedBatch(self, gaps)

    def execute_scaffolds(self, scaffolds_text, k, solid=2, max_fuz=10, nb_cores=1, max_mem_gb=20.0,
                          reads_label="reads.fa", filled_label="filled.fa"):
        lib = load_library()
        o = g2s_run_opts(k, solid, max_fuz, nb_cores, max_mem_gb)
        fa, lg = _VP(), _VP()
        gaps, filled = C.c_int32(0), C.c_int32(0)
        _check(lib.g2s_execute_scaffolds(self.h, C.byref(o), reads_label.encode(), filled_label.encode(),
                                         scaffolds_text.encode("ascii"), C.byref(fa), C.byref(lg), C.byref(gaps),
                                         C.byref(filled)))
        return _take_text(fa), _take_text(lg), gaps.value, filled.value

    def execute_scaffolds_stream(self, scaffolds_text, k, chunk_gaps, solid=2, max_fuz=10, nb_cores=1, max_mem_gb=20.0,
                                 reads_label="reads.fa", filled_label="filled.fa"):
        """g2s_execute_scaffolds_stream; returns (fasta pieces, log pieces, gaps, filled): one piece per batch."""
        lib = load_library()
        o = g2s_run_opts(k, solid, max_fuz, nb_cores, max_mem_gb)
        fa, lg = [], []
        on_fa = TEXT_FN(lambda t, n, u: fa.append(C.string_at(t, n).decode("ascii")))
        on_lg = TEXT_FN(lambda t, n, u: lg.append(C.string_at(t, n).decode("ascii")))
        gaps, filled = C.c_int32(0), C.c_int32(0)
        _check(lib.g2s_execute_scaffolds_stream(self.h, C.byref(o), reads_label.encode(), filled_label.encode(),
                                                scaffolds_text.encode("ascii"), chunk_gaps, on_fa, on_lg, None,
                                                C.byref(gaps), C.byref(filled)))
        return fa, lg, gaps.value, filled.value

    def execute_single(self, left, right, length, k, solid=2, max_fuz=10, max_mem_gb=20.0,
                       reads_label="reads.fa", filled_label="filled.fa"):
        lib = load_library()
        o = g2s_run_opts(k, solid, max_fuz, 1, max_mem_gb)
        fa, lg = _VP(), _VP()
        _check(lib.g2s_execute_single(self.h, C.byref(o), reads_label.encode(), filled_label.encode(),
                                      left.encode("ascii"), right.encode("ascii"), length, C.byref(fa), C.byref(lg)))
        return _take_text(fa), _take_text(lg)

    def destroy(self):
        if self.h:
            load_library().g2s_session_destroy(self.h)
            self.h = None


def team_fill(sessions, gaps, group_size=0, want_timing=False, prepared=None, pinned=False):
    """g2s_team_fill: the sessions (one or more per device) share one gap list; results equal
    sessions[0].fill_batch(gaps).  `prepared` = (arr, keep, arena, res) from a previous call to
    skip the marshalling (bench).  pinned: results and arena in g2s_host_alloc memory (every session's kernels then
    write its own group's results there: phase D3 sharded over the team); the buffers are not freed (tests)."""
    lib = load_library()
    if prepared is None:
        arr, keep = _gap_array(gaps)
        nbytes = lib.g2s_team_arena_bytes(sessions[0].h, arr, len(gaps))
        if pinned:
            arena = HostBuffer(max(1, nbytes))
            rbuf = HostBuffer(C.sizeof(g2s_result) * max(1, len(gaps)))
            res = rbuf.array(g2s_result, max(1, len(gaps)))
            hs = (_VP * len(sessions))(*[s.h for s in sessions])
            t = g2s_timing()
            try:
                _check(lib.g2s_team_fill(hs, len(sessions), arr, len(gaps), group_size, res, C.cast(arena.p, C.c_char_p), nbytes, C.byref(t)))
                raw = arena.raw
                out = [FillResult(res[i], raw) for i in range(len(gaps))]
            finally:
                arena.free()
                rbuf.free()
            return (out, t) if want_timing else out
        arena = C.create_string_buffer(max(1, nbytes))
        res = (g2s_result * max(1, len(gaps)))()
        prepared = (arr, keep, arena, res, nbytes)
    arr, keep, arena, res, nbytes = prepared
    hs = (_VP * len(sessions))(*[s.h for s in sessions])
    t = g2s_timing()
    _check(lib.g2s_team_fill(hs, len(sessions), arr, len(gaps), group_size, res, arena, nbytes, C.byref(t)))
    if want_timing == "raw":
        return prepared, t
    raw = arena.raw
    out = [FillResult(res[i], raw) for i in range(len(gaps))]
    return (out, t) if want_timing else out


class PreparedBatch:
    def __init__(self, session, gaps):
        lib = load_library()
        self.session = session
        self.n = len(gaps)
        self._arr, self._keep = _gap_array(gaps)
        self.h = _VP()
        _check(lib.g2s_batch_prepare(session.h, self._arr, self.n, C.byref(self.h)))
        self.nbytes = lib.g2s_batch_arena_bytes(self.h)
        self.arena = C.create_string_buffer(max(1, self.nbytes))
        self.res = (g2s_result * max(1, self.n))()

    def run(self):
        _check(load_library().g2s_batch_run(self.h, self.res, self.arena, self.nbytes))

    def timing(self):
        t = g2s_timing()
        _check(load_library().g2s_batch_timing(self.h, C.byref(t)))
        return t

    def results(self):
        raw = self.arena.raw
        return [FillResult(self.res[i], raw) for i in range(self.n)]

    def free(self):
        if self.h:
            load_library().g2s_batch_free(self.h)
            self.h = None


def test_post_gap(graph, params, gap, states, c_count, lengths, reached_j, final_d, seed, skip):
    """TEST HOOK binding (host half of phase D on a supplied DP table)."""
    lib = load_library()
    arr, keep = _gap_array([gap])
    n = len(states)
    nodes = (C.c_uint32 * max(1, n))(*[s[0] for s in states])
    depths = (C.c_int32 * max(1, n))(*[s[1] for s in states])
    counts = (C.c_uint32 * max(1, n))(*[s[2] for s in states])
    lens = (C.c_int32 * 2)(*(list(lengths) + [0, 0])[:2])
    res = g2s_result()
    buf = C.create_string_buffer(gap.gap_len + graph.k + params.d_err + gap.lmf + gap.rmf + 3)
    _check(lib.g2s_test_post_gap(graph.h, C.byref(params), arr, n, nodes, depths, counts, c_count, len(lengths), lens,
                                 reached_j, final_d, seed, skip, C.byref(res), buf))
    return FillResult(res, buf.raw)


def test_post_closure(graph, params, gap, records, xp, c_count, lengths, reached_j, final_d, seed, skip):
    """TEST HOOK binding: host D2 + D3 on a closure in the kernels' output layout.
    records: list of (node, count, meta, pred) with pred as a signed int."""
    lib = load_library()
    arr, keep = _gap_array([gap])
    n = len(records)
    flat = (C.c_uint32 * max(1, 4 * n))()
    for i, (node, cnt, meta, pred) in enumerate(records):
        flat[4 * i], flat[4 * i + 1], flat[4 * i + 2], flat[4 * i + 3] = node, cnt, meta, pred & 0xFFFFFFFF
    xs = (C.c_uint64 * max(1, len(xp)))(*xp)
    lens = (C.c_int32 * 2)(*(list(lengths) + [0, 0])[:2])
    res = g2s_result()
    buf = C.create_string_buffer(gap.gap_len + graph.k + params.d_err + gap.lmf + gap.rmf + 3)
    _check(lib.g2s_test_post_closure(graph.h, C.byref(params), arr, n, flat, len(xp), xs, c_count, len(lengths), lens,
                                     reached_j, final_d, seed, skip, C.byref(res), buf))
    return FillResult(res, buf.raw)


def test_post_segments(graph, params, gap, segs, c_count, lengths, reached_j, final_d, seed, skip):
    """TEST HOOK binding: host D2 + D3 directly on closure segments; returns (FillResult, on_segments)."""
    lib = load_library()
    arr, keep = _gap_array([gap])
    flat = (C.c_uint32 * max(1, 8 * len(segs)))()
    for i, rec in enumerate(segs):
        for q in range(8):
            flat[8 * i + q] = rec[q] & 0xFFFFFFFF
    lens = (C.c_int32 * 2)(*(list(lengths) + [0, 0])[:2])
    res = g2s_result()
    on = C.c_int32(0)
    buf = C.create_string_buffer(gap.gap_len + graph.k + params.d_err + gap.lmf + gap.rmf + 3)
    _check(lib.g2s_test_post_segments(graph.h, C.byref(params), arr, len(segs), flat, c_count, len(lengths), lens,
                                      reached_j, final_d, seed, skip, C.byref(res), buf, C.byref(on)))
    return FillResult(res, buf.raw), bool(on.value)


def test_seg_expand(graph, params, gap, segs, lengths, reached_j, n_records, n_xp):
    """TEST HOOK binding: closure segments (8 words each) -> ([(node, cnt, meta, pred)], sorted xp)."""
    lib = load_library()
    arr, keep = _gap_array([gap])
    flat = (C.c_uint32 * max(1, 8 * len(segs)))()
    for i, rec in enumerate(segs):
        for q in range(8):
            flat[8 * i + q] = rec[q] & 0xFFFFFFFF
    lens = (C.c_int32 * 2)(*(list(lengths) + [0, 0])[:2])
    out = (C.c_uint32 * max(1, 4 * n_records))()
    xs = (C.c_uint64 * max(1, n_xp))()
    _check(lib.g2s_test_seg_expand(graph.h, C.byref(params), arr, len(segs), flat, len(lengths), lens, reached_j,
                                   n_records, out, n_xp, xs))
    recs = [(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3] - (1 << 32) if out[4 * i + 3] >> 31 else out[4 * i + 3])
            for i in range(n_records)]
    return recs, sorted(xs[i] for i in range(n_xp))


def test_graph_tables(graph):
    """TEST HOOK binding: (succ, ustart) as flat lists of ints: successor table (2n x 4) and bitmap words."""
    n = graph.num_kmers
    succ = (C.c_uint32 * max(1, 8 * n))()
    words = (C.c_uint64 * max(1, (n + 63) // 64))()
    _check(load_library().g2s_test_graph_tables(graph.h, succ, words))
    return succ, words


def test_worker_pool(threads, rounds, n):
    """TEST HOOK binding: stress the host worker pool; raises G2SError on a lost or repeated task."""
    _check(load_library().g2s_test_worker_pool(threads, rounds, n))


def test_group_queue(nworkers, n, group_size):
    """TEST HOOK binding: the dispatcher's shared group counter with host threads in place of
    sessions; returns the worker each gap was handed to (raises G2SError on a lost or doubled gap)."""
    owner = (C.c_int32 * max(1, n))()
    _check(load_library().g2s_test_group_queue(nworkers, n, group_size, owner))
    return [owner[i] for i in range(n)]


def test_device_rand(device, seed, skip, n):
    """TEST HOOK binding: the same n values from the device's generator (g2s_rand_fill)."""
    out = (C.c_int32 * max(1, n))()
    _check(load_library().g2s_test_device_rand(device, seed, skip, n, out))
    return [out[i] for i in range(n)]


def test_d3_tables(device, segs, n_len, len0, len1, start_seg, rnd, base, R, dmin, dspread):
    """TEST HOOK binding (g2s_test_d3_tables): the product's kernel g2s_d3_tables_waves for one designed gap.  segs: a list of
    (depth | len << 16, parents 0-1, parents 2-3, flags); rnd: the stream's raw words (nothing exists behind them).
    Returns (entries, bad, anomalies): the table entry and the bad verdict of every deviation 0 .. R, the list's counter."""
    flat = [w for s in segs for w in s]
    sa = (C.c_uint32 * max(1, len(flat)))(*flat)
    ra = (C.c_uint32 * max(1, len(rnd)))(*rnd)
    ent, bad, anom = (C.c_uint16 * (R + 1))(), (C.c_uint8 * (R + 1))(), C.c_uint32()
    _check(load_library().g2s_test_d3_tables(device, sa, len(segs), n_len, len0, len1, start_seg, ra, len(rnd), base, R, dmin,
                                             dspread, ent, bad, C.byref(anom)))
    return list(ent), list(bad), anom.value


def test_d3_chain_launches():
    """TEST HOOK binding: lists of this process that took phase D3's short route (the chain walked by the trace kernel)."""
    return int(load_library().g2s_test_d3_chain_launches())


def test_group_queue_slow(nworkers, n, group_size, slow_worker, slow_us):
    """TEST HOOK binding: the group counter with one worker that is slow_us microseconds slower per group."""
    owner = (C.c_int32 * max(1, n))()
    _check(load_library().g2s_test_group_queue_slow(nworkers, n, group_size, slow_worker, slow_us, owner))
    return [owner[i] for i in range(n)]


def test_rand_skip(seed, skip, n):
    """TEST HOOK binding: the same values reached by a jump over `skip` values (g2s_share_end's way)."""
    out = (C.c_int32 * max(1, n))()
    _check(load_library().g2s_test_rand_skip(seed, skip, n, out))
    return [out[i] for i in range(n)]


def test_rand_stream(seed, skip, n):
    """TEST HOOK binding: n values of the product's rand() stream after srand(seed), skipping `skip`."""
    out = (C.c_int32 * max(1, n))()
    _check(load_library().g2s_test_rand_stream(seed, skip, n, out))
    return [out[i] for i in range(n)]


def reach_radius(gap, d_err):
    """The sound radius of g2s_graph_build_pool_reach for a fill of `gap` with -dist-error `d_err`:
    max(0, gap_len + d_err) + lmf + rmf, the depth bound of the reference's search."""
    return max(0, gap.gap_len + d_err) + gap.lmf + gap.rmf


def test_last_pool_reach():
    """g2s_test_last_pool_reach: dict(reach_sets, full_kmers (None when not counted), kept_kmers, levels, on_device) of
    the last pooled build with a reach record"""
    a, b, d = C.c_uint64(), C.c_uint64(), C.c_uint64()
    known, on = C.c_int(), C.c_int()
    lv = C.c_uint32()
    _check(load_library().g2s_test_last_pool_reach(C.byref(a), C.byref(b), C.byref(known), C.byref(d), C.byref(lv), C.byref(on)))
    return dict(reach_sets=a.value, full_kmers=b.value if known.value else None, kept_kmers=d.value, levels=lv.value,
                on_device=on.value)


def test_seg_back_record(graph, device, node):
    """TEST HOOK binding (g2s_test_seg_back_record): ([four words], steps) — what the segment tier reads to walk backwards
    from the oriented node `node`: the far end's predecessors in slot order, orientation bits flipped, and the walk's length"""
    out = (C.c_uint32 * 5)()
    _check(load_library().g2s_test_seg_back_record(graph.h, device, node, out))
    return list(out[:4]), out[4]


def test_last_pool_build():
    """g2s_test_last_pool_build: dict(own_positions, shared_positions, keys_sorted, on_device) of the last pooled build"""
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    _check(load_library().g2s_test_last_pool_build(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return dict(own_positions=a.value, shared_positions=b.value, keys_sorted=c.value, on_device=d.value)


def test_last_solid_count():
    """g2s_test_last_solid_count: dict(positions, passes, refined_bins, max_pass_keys, solid, on_device) of the last
    single-graph build's solid k-mer count (passes == 0: the one-sort device count, or the host count)"""
    pos, mx, so = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ps, rf, on = C.c_uint32(), C.c_uint32(), C.c_int()
    _check(load_library().g2s_test_last_solid_count(C.byref(pos), C.byref(ps), C.byref(rf), C.byref(mx), C.byref(so), C.byref(on)))
    return dict(positions=pos.value, passes=ps.value, refined_bins=rf.value, max_pass_keys=mx.value, solid=so.value,
                on_device=on.value)


def test_plan_passes(hist, cap):
    """TEST HOOK binding (g2s_test_plan_passes): (the first bin of every pass, the first bin with more than `cap` keys or
    None) for the histogram `hist` cut greedily into key-range passes of at most `cap` keys"""
    nb = len(hist)
    h = (C.c_uint64 * max(1, nb))(*hist)
    first = (C.c_uint32 * max(1, nb))()
    n, over = C.c_uint32(), C.c_uint32()
    _check(load_library().g2s_test_plan_passes(h, nb, cap, first, nb, C.byref(n), C.byref(over)))
    assert n.value <= nb
    return list(first[:n.value]), (over.value if over.value < nb else None)


def test_filter_join(ref_id, pos, end, flag, h_own, h_mate, max_span, bits, windows, max_pairs, device=-1, threads=1):
    """TEST HOOK binding: the joins of the batched read filter on the caller's rows; `windows` holds three
    (tid, beg, end) a gap.  device < 0: the host joins on `threads` threads; otherwise the device joins (no host path
    in their place).  Returns (the join's code, list 1, list 2, g2s_filter_last_error's text) with the lists as
    (gap, row) tuples; nothing is raised, the code is the caller's to check."""
    lib = load_library()
    nr, n = len(pos), len(windows) // 3
    assert len(windows) == 3 * n and all(len(x) == nr for x in (ref_id, end, flag, h_own, h_mate))
    flat = [v for w in windows for v in w]
    args = [(C.c_int32 * max(1, nr))(*ref_id), (C.c_int32 * max(1, nr))(*pos), (C.c_int64 * max(1, nr))(*end),
            (C.c_uint32 * max(1, nr))(*flag), (C.c_uint64 * max(1, nr))(*h_own), (C.c_uint64 * max(1, nr))(*h_mate)]
    win = (C.c_int64 * max(1, len(flat)))(*flat)
    cap1 = cap2 = 1 << 16
    while True:
        l1, l2 = (C.c_uint64 * cap1)(), (C.c_uint64 * cap2)()
        n1, n2 = C.c_uint64(0), C.c_uint64(0)
        rc = lib.g2s_test_filter_join(device, threads, nr, *args, max_span, bits, n, win, max_pairs, l1, cap1,
                                      C.byref(n1), l2, cap2, C.byref(n2))
        if rc != G2S_OK or (n1.value <= cap1 and n2.value <= cap2):
            break
        cap1, cap2 = max(cap1, n1.value), max(cap2, n2.value)
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    return rc, [(x >> 32, x & 0xFFFFFFFF) for x in l1[:n1.value]], [(x >> 32, x & 0xFFFFFFFF) for x in l2[:n2.value]], msg


def reads_text(data, device=-1, piece_bytes=0):
    """TEST HOOK binding (g2s_test_reads_text): the build's text (every sequence followed by N) of one read file in
    memory, plain, gzip or BGZF, or of one BAM file.  device -1: the host loader (zlib, parse_fastx; the reader's walk
    for BAM); -2: the kernels' state machine walked on the host (BAM: as -1); >= 0: the kernels on that device in pieces
    (BAM: windows) of `piece_bytes` raw bytes.  Raises G2SError."""
    lib = load_library()
    data = bytes(data)
    cap = max(1 << 12, 2 * len(data))
    while True:
        out = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        _check(lib.g2s_test_reads_text(data, len(data), device, piece_bytes, out, cap, C.byref(n)))
        if n.value <= cap:
            return bytes(out[:n.value])
        cap = n.value


def last_reads_load():
    """TEST HOOK binding (g2s_test_last_reads_load): dict(files, raw_bytes, positions, records, pieces, on_device,
    inflate, grows) of the process's last Graph.from_files or reads_text; inflate is a list with one of "none", "zlib",
    "device", "mixed", "device-gzip" a file (the last only when set_device_gzip or G2S_DEVICE_GZIP asked for it)"""
    f, rb, ps, rc, pc, gr = (C.c_uint64() for _ in range(6))
    on = C.c_int()
    _check(load_library().g2s_test_last_reads_load(C.byref(f), None, None, None, None, None, None, 0, None))
    how = (C.c_int * max(1, f.value))()
    _check(load_library().g2s_test_last_reads_load(C.byref(f), C.byref(rb), C.byref(ps), C.byref(rc), C.byref(pc), C.byref(on),
                                                   how, f.value, C.byref(gr)))
    return dict(files=f.value, raw_bytes=rb.value, positions=ps.value, records=rc.value, pieces=pc.value,
                on_device=on.value, inflate=[("none", "zlib", "device", "mixed", "device-gzip")[x] for x in how[:f.value]], grows=gr.value)


BAM_READS_REASONS = ("kernels", "not asked", "rows anomaly", "over the cap", "hip")


def last_reads_bam():
    """TEST HOOK binding (g2s_test_last_reads_bam): dict(files, kept, skipped, kernels, reason, anomaly) of the BAM
    files in the process's last Graph.from_files or reads_text; reason is one of BAM_READS_REASONS, anomaly the
    RowsAnomaly (csrc/bam_rows.h) behind "rows anomaly" """
    f, kept, skipped = C.c_uint64(), C.c_uint64(), C.c_uint64()
    kernels, reason, anomaly = C.c_int(), C.c_int(), C.c_int()
    _check(load_library().g2s_test_last_reads_bam(C.byref(f), C.byref(kept), C.byref(skipped), C.byref(kernels),
                                                  C.byref(reason), C.byref(anomaly)))
    return dict(files=f.value, kept=kept.value, skipped=skipped.value, kernels=kernels.value,
                reason=BAM_READS_REASONS[reason.value], anomaly=anomaly.value)


def last_reads_bam_stream():
    """TEST HOOK binding (g2s_test_last_reads_bam_stream): dict(streamed_files, windows, peak_device_bytes) of the
    streaming form of the BAM read route in the process's last Graph.from_files or reads_text: the BAM files whose text
    it wrote, their walk windows, the largest device footprint counted against the bound; zeros when none was streamed"""
    f, w, peak = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(load_library().g2s_test_last_reads_bam_stream(C.byref(f), C.byref(w), C.byref(peak)))
    return dict(streamed_files=f.value, windows=w.value, peak_device_bytes=peak.value)


GZIP_OUTCOMES = ("done", "too few starts", "boundary mismatch", "slot full", "corrupt", "trailer", "memory", "hip", "header")


def set_device_gzip(mode=1):
    """g2s_reads_set_device_gzip: 1 asks for the chunked device inflate of plain gzip read files in every later
    Graph.from_files of the process, 0 forbids it, -1 follows G2S_DEVICE_GZIP.  Returns the previous mode."""
    return load_library().g2s_reads_set_device_gzip(int(mode))


def gzip_inflate(data, device=-1, chunk_bytes=0, window_chunks=0):
    """TEST HOOK binding (g2s_test_gzip_inflate): a whole gzip file inflated on `device` (>= 0: the kernels; -1: zlib;
    -2: the kernels' algorithm compiled for the host) in chunks of chunk_bytes and windows of window_chunks chunks (0: the
    whole file).  Returns (bytes, outcome): outcome one of GZIP_OUTCOMES, and anything but "done" comes with no bytes.
    Raises G2SError (device -1: a damaged file, with zlib's message)."""
    lib = load_library()
    data = bytes(data)
    cap = max(1 << 16, 8 * len(data))
    while True:
        out = (C.c_uint8 * cap)()
        n, oc = C.c_size_t(0), C.c_int(0)
        _check(lib.g2s_test_gzip_inflate(data, len(data), device, chunk_bytes, window_chunks, out, cap, C.byref(n), C.byref(oc)))
        if n.value <= cap:
            return bytes(out[:n.value]), GZIP_OUTCOMES[oc.value]
        cap = n.value


def last_reads_gzip():
    """TEST HOOK binding (g2s_test_last_reads_gzip): dict(files, windows, chunks, starts_found, absorbed, members,
    outcome (one of GZIP_OUTCOMES), peak_device_bytes) of the chunked device inflate in the process's last
    Graph.from_files, reads_text or gzip_inflate"""
    v = [C.c_uint64() for _ in range(7)]
    oc = C.c_int()
    _check(load_library().g2s_test_last_reads_gzip(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(v[4]),
                                                   C.byref(v[5]), C.byref(oc), C.byref(v[6])))
    return dict(files=v[0].value, windows=v[1].value, chunks=v[2].value, starts_found=v[3].value, absorbed=v[4].value,
                members=v[5].value, outcome=GZIP_OUTCOMES[oc.value], peak_device_bytes=v[6].value)


def bgzf_inflate(data, device=-1):
    """TEST HOOK binding (g2s_test_bgzf_inflate): a whole BGZF file inflated on `device` (>= 0: the kernel; -1: zlib;
    -2: the kernel's decoder compiled for the host).  Returns (code, bytes, bad_member, g2s_filter_last_error's text);
    nothing is raised, the code is the caller's to check."""
    lib = load_library()
    data = bytes(data)
    cap = max(1 << 16, 4 * len(data))
    while True:
        out = (C.c_uint8 * cap)()
        n, bad = C.c_size_t(0), C.c_int64(-1)
        rc = lib.g2s_test_bgzf_inflate(data, len(data), device, out, cap, C.byref(n), C.byref(bad))
        if rc != G2S_OK or n.value <= cap:
            break
        cap = n.value
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    return rc, (bytes(out[:n.value]) if rc == G2S_OK else b""), bad.value, msg


def last_filter_inflate():
    """TEST HOOK binding (g2s_test_last_filter_inflate): dict(on_device, members, bytes_in, bytes_out, ms_pass_a_inflate,
    ms_pass_b_inflate) of the process's last batched filter call"""
    d, m, bi, bo, a, b = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double()
    _check(load_library().g2s_test_last_filter_inflate(C.byref(d), C.byref(m), C.byref(bi), C.byref(bo), C.byref(a), C.byref(b)))
    return dict(on_device=d.value, members=m.value, bytes_in=bi.value, bytes_out=bo.value, ms_pass_a_inflate=a.value,
                ms_pass_b_inflate=b.value)


def bam_rows(data, device=-1, window=0, kept=False):
    """TEST HOOK binding (g2s_test_bam_rows): pass A alone on a BAM file in memory, by the host walk (device -1) or by the
    kernels on `device`, `window` bytes at a time (0: the reader's window).  Returns (code, rows, g2s_filter_last_error's
    text) with rows = dict(ref_id, pos, end, flag, h_own, h_mate: lists in file order; total, read_length, max_span), or
    None when the code is not G2S_OK; nothing is raised, the code is the caller's to check.  kept=True
    (g2s_test_bam_rows_kept): pass A as one-pass mode runs it, the inflated file kept in one device allocation."""
    lib = load_library()
    hook = lib.g2s_test_bam_rows_kept if kept else lib.g2s_test_bam_rows
    data = bytes(data)
    cap = 1 << 12
    while True:
        arr = [(C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint64 * cap)(),
               (C.c_uint64 * cap)()]
        total, rl, span = C.c_uint64(0), C.c_int32(0), C.c_int64(0)
        rc = hook(data, len(data), device, window, cap, *arr, C.byref(total), C.byref(rl), C.byref(span))
        if rc != G2S_OK or total.value <= cap:
            break
        cap = total.value
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    if rc != G2S_OK:
        return rc, None, msg
    n = total.value
    names = ("ref_id", "pos", "end", "flag", "h_own", "h_mate")
    rows = {k: list(a[:n]) for k, a in zip(names, arr)}
    rows.update(total=n, read_length=rl.value, max_span=span.value)
    return rc, rows, msg


def name_hash(name, which):
    """TEST HOOK binding (g2s_test_name_hash): (std::hash<std::string> of name + "/1" or "/2", the same from
    csrc/name_hash.h); `name` is the l_name bytes of a record, of which the part in front of the first NUL counts."""
    a, b = C.c_uint64(), C.c_uint64()
    name = bytes(name)
    _check(load_library().g2s_test_name_hash(name, len(name), which, C.byref(a), C.byref(b)))
    return a.value, b.value


def last_filter_rows():
    """TEST HOOK binding (g2s_test_last_filter_rows): dict(on_device, windows, records, candidates, anomaly) of pass A in
    the process's last batched filter call or bam_rows call"""
    d, w, r, c, a = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    _check(load_library().g2s_test_last_filter_rows(C.byref(d), C.byref(w), C.byref(r), C.byref(c), C.byref(a)))
    return dict(on_device=d.value, windows=w.value, records=r.value, candidates=c.value, anomaly=a.value)


def filter_set_one_pass(mode):
    """g2s_filter_set_one_pass: 1 asks for one-pass mode in every later batched filter call of the process, 0 forbids it,
    -1 follows G2S_FILTER_ONE_PASS.  Returns the previous mode."""
    return load_library().g2s_filter_set_one_pass(int(mode))


TEXT_REASONS = ("on the device", "not asked", "no device rows", "over the cap", "allocation or HIP failure",
                "a planned capacity of the store route overflowed")


def last_filter_text():
    """TEST HOOK binding (g2s_test_last_filter_text): dict(one_pass, reason (index into TEXT_REASONS), reads, bytes,
    resident_bytes) of pass B in the process's last batched filter call"""
    o, r, n, b, rb = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(load_library().g2s_test_last_filter_text(C.byref(o), C.byref(r), C.byref(n), C.byref(b), C.byref(rb)))
    return dict(one_pass=o.value, reason=r.value, reads=n.value, bytes=b.value, resident_bytes=rb.value)


def bam_text(data, rows, device=-1, names=True, fasta=False, store=False, window=0):
    """TEST HOOK binding (g2s_test_bam_text): pass B alone on a BAM file in memory for the records `rows` (indices in file
    order), by the host walk (device -1) or by the kernels on `device`.  Returns (code, dict(bases, base_off, names,
    name_off) or None, g2s_filter_last_error's text): the pool's arrays of the selected records in file order, or with
    fasta=True their FASTA records in `bases`; nothing is raised, the code is the caller's to check.  store=True
    (g2s_test_bam_text_store): pass A in store form, the row kernels `window` bytes at a time (0: the reader's window)."""
    lib = load_library()
    data = bytes(data)
    rows = list(rows)
    arr = (C.c_uint32 * max(1, len(rows)))(*rows)
    bcap, ncap, ocap = 1 << 16, 1 << 12, len(set(rows)) + 1
    while True:
        B, N = (C.c_uint8 * bcap)(), (C.c_uint8 * ncap)()
        bo, no = (C.c_uint64 * ocap)(), (C.c_uint64 * ocap)()
        bn, nn, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        tail = (arr, len(rows), int(names), int(fasta), B, bcap, C.byref(bn), N, ncap, C.byref(nn), bo, no, ocap, C.byref(nr))
        if store:
            rc = lib.g2s_test_bam_text_store(data, len(data), device, window, *tail)
        else:
            rc = lib.g2s_test_bam_text(data, len(data), device, *tail)
        if rc != G2S_OK or (bn.value <= bcap and nn.value <= ncap and nr.value + 1 <= ocap):
            break
        bcap, ncap, ocap = max(bcap, bn.value), max(ncap, nn.value), max(ocap, nr.value + 1)
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    if rc != G2S_OK:
        return rc, None, msg
    m = nr.value + 1
    return rc, dict(bases=bytes(B[:bn.value]), base_off=list(bo[:m]), names=bytes(N[:nn.value]),
                    name_off=list(no[:m]) if names and not fasta else None), msg


def filter_store_plan(data):
    """TEST HOOK binding (g2s_test_filter_store_plan): the store route's plan for a BAM file in memory, on the host.
    Returns (code, dict(sample_records, sample_bytes, sample_stored, rows_cap, store_cap, need) or None,
    g2s_filter_last_error's text); G2S_FILTER_STORE_SAMPLE is read."""
    lib = load_library()
    data = bytes(data)
    v = [C.c_uint64() for _ in range(6)]
    rc = lib.g2s_test_filter_store_plan(data, len(data), *[C.byref(x) for x in v])
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    if rc != G2S_OK:
        return rc, None, msg
    keys = ("sample_records", "sample_bytes", "sample_stored", "rows_cap", "store_cap", "need")
    return rc, dict(zip(keys, (x.value for x in v))), msg


def bam_store(data, device=-1, window=0):
    """TEST HOOK binding (g2s_test_bam_store): the store of a BAM file in memory, by the host model (device -1) or by the
    kernels on `device` behind the row kernels, `window` bytes at a time (0: the reader's window).  Returns (code,
    (store bytes, [every record's offset]) or None, g2s_filter_last_error's text); nothing is raised."""
    lib = load_library()
    data = bytes(data)
    scap, ocap = 1 << 16, 1 << 10
    while True:
        S, O = (C.c_uint8 * scap)(), (C.c_uint64 * ocap)()
        sn, on = C.c_uint64(0), C.c_uint64(0)
        rc = lib.g2s_test_bam_store(data, len(data), device, window, S, scap, C.byref(sn), O, ocap, C.byref(on))
        if rc != G2S_OK or (sn.value <= scap and on.value <= ocap):
            break
        scap, ocap = max(scap, sn.value), max(ocap, on.value)
    msg = (lib.g2s_filter_last_error() or b"").decode("utf-8", "replace")
    if rc != G2S_OK:
        return rc, None, msg
    return rc, (bytes(S[:sn.value]), list(O[:on.value])), msg


def last_filter_store():
    """TEST HOOK binding (g2s_test_last_filter_store): dict(used, records, store_bytes, store_cap, rows_cap, device_bytes,
    overflow) of the store route in the process's last batched filter call; overflow is 0 none, 1 the rows, 2 the store"""
    u, o = C.c_int(), C.c_int()
    v = [C.c_uint64() for _ in range(5)]
    _check(load_library().g2s_test_last_filter_store(C.byref(u), *[C.byref(x) for x in v], C.byref(o)))
    keys = ("records", "store_bytes", "store_cap", "rows_cap", "device_bytes")
    return dict(zip(keys, (x.value for x in v)), used=u.value, overflow=o.value)
