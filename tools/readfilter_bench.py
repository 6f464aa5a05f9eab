"""tools/readfilter_bench.py — the read extraction of libraries mode, three ways, on one simulated library:

  per_gap   g2s_filter_reads once a gap (what Gap2Seq-libraries did before g2s_filter_reads_gaps), timed on the first
            --loop-gaps gaps and extrapolated linearly to all of them (every call inflates the file twice)
  host      g2s_filter_reads_gaps with the joins on host threads (device -1)
  device    g2s_filter_reads_gaps with the joins on the GPU, with its laps: the first call of the process (HIP's
            start-up falls into its first device lap) and a second one; the file is inflated on the GPU too
  device_host_inflate   (--host-inflate) the same with G2S_HOST_INFLATE=1: zlib on host threads, the joins on the GPU
  --one-pass            asks for one-pass mode in every batched call (g2s_filter_set_one_pass(1)): the device legs then
                        report file_passes 1, and every leg says whether pass B ran on the device (text_on_device)
  --resident-cap BYTES  G2S_FILTER_RESIDENT_CAP for the legs: under the whole stream's need (the inflated file and 52 bytes
                        for every 36 of them) one-pass mode takes the store route (store.used 1) when its need fits
  --store 0|1           G2S_FILTER_STORE for the legs: 1 takes the store route even when the whole stream fits, 0 never
  --handover            nothing of the above: BAM file to uploaded set graph, the hand-over of the reads two ways, --calls
                        times each in turn after one untimed call of each (k --k, every gap one set, one set in 50 flagged
                        for the unmapped reads, no reach records, one-pass mode asked for):
                          pool    g2s_filter_reads_gaps_pool (names, unmapped), the pointer and length tables of
                                  Gap2Seq-libraries, g2s_graph_build_pool_reach, g2s_graph_upload
                          dpool   g2s_filter_reads_gaps_dpool, g2s_graph_build_dpool_reach, g2s_graph_upload
                        with each leg's laps (filter, tables, build, upload), the device bytes the pool holds, what
                        g2s_test_last_dpool said, and whether the two graphs have the same sets

Every batched run carries the store route's hook (g2s_test_last_filter_store: used, records, store_bytes, store_cap,
rows_cap, device_bytes, overflow) under "store".  Every run also carries the reader's own laps (g2s_test_last_filter_inflate): whether the file was inflated on the
device and the time inside the reader's refills in pass A and pass B.

Prints one JSON line.  The library is tests/bamwriter.simulate_library's, about --pairs read pairs on 10 scaffolds,
with --gaps gaps at random breakpoints; the same gaps for all three, on the coordinate-sorted file and on the same
records shuffled (where the host joins sort their index, which a sorted file spares them).

  python tools/readfilter_bench.py [--pairs 1000000] [--gaps 1000] [--loop-gaps 20] [--device 0] [--threads 0]
                                   [--host-inflate] [--one-pass] [--resident-cap BYTES] [--store 0|1]
                                   [--handover [--calls 6] [--k 31]]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bamwriter as BW  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402


def handover(a, bam, gaps, mean, sd):
    """BAM file to uploaded set graph through a host pool and through a device-held pool, alternating"""
    import numpy as np
    lib = P.load_library()
    P.filter_set_one_pass(1)
    arr = P._filter_gap_array(gaps)
    n = len(gaps)
    opts = P.g2s_filter_opts(mean, sd, 0, -1, -1, 0, a.threads, b"")
    flags = (C.c_uint8 * n)(*[1 if i % 50 == 0 else 0 for i in range(n)])
    PP = C.POINTER

    def finish(h, t, laps, sets):
        laps["build"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        if a.device >= 0:   # (a dry run on the host has nowhere to upload to)
            P._check(lib.g2s_graph_upload(h, a.device))
        laps["upload"] = (time.perf_counter() - t) * 1e3
        g = P.Graph(h)
        if sets is not None:
            sets.append((g.num_kmers, [g.set_nodes(i) for i in range(0, n, max(1, n // 64))]))
        g.free()

    def run_pool(sets=None):
        laps, t0 = {}, time.perf_counter()
        out, tot = PP(P.g2s_read_pool)(), C.c_int64(0)
        rc = lib.g2s_filter_reads_gaps_pool_mem(bam, len(bam), C.byref(opts), arr, n, a.device, 1, 1, C.byref(out), C.byref(tot), None)
        assert rc == P.G2S_OK, lib.g2s_filter_last_error()
        laps["filter"] = (time.perf_counter() - t0) * 1e3
        t = time.perf_counter()
        p = out.contents
        off = np.ctypeslib.as_array(p.base_off, shape=(p.n_reads + 1,))
        ptrs = (off[:-1] + np.uint64(C.cast(p.bases, C.c_void_p).value)).astype(np.uint64)
        lens = np.diff(off).astype(np.uint64)
        laps["tables"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        h = C.c_void_p()
        P._check(lib.g2s_graph_build_pool_reach(C.cast(ptrs.ctypes.data, PP(C.c_char_p)), C.cast(lens.ctypes.data, PP(C.c_uint64)),
                                                p.n_reads, p.gap_begin, p.gap_read, p.unmapped_read, p.n_unmapped, flags, n,
                                                a.k, 2, 0, None, None, C.byref(h)))
        lib.g2s_read_pool_free(out)
        finish(h, t, laps, sets)
        laps["whole"] = (time.perf_counter() - t0) * 1e3
        return laps

    def run_dpool(sets=None):
        laps, t0 = {}, time.perf_counter()
        out, tot = C.c_void_p(), C.c_int64(0)
        rc = lib.g2s_filter_reads_gaps_dpool_mem(bam, len(bam), C.byref(opts), arr, n, a.device, 1, C.byref(out), C.byref(tot), None)
        assert rc == P.G2S_OK, lib.g2s_filter_last_error()
        laps["filter"] = (time.perf_counter() - t0) * 1e3
        held = P.test_last_dpool()
        laps["tables"] = 0.0
        t = time.perf_counter()
        p = lib.g2s_device_pool_view(out).contents
        pools = (C.c_void_p * 1)(out.value)
        h = C.c_void_p()
        P._check(lib.g2s_graph_build_dpool_reach(pools, 1, p.gap_begin, p.gap_read, p.unmapped_read, p.n_unmapped, flags, n, a.k,
                                                 2, 0, None, None, C.byref(h)))
        info = dict(device=lib.g2s_device_pool_device(out), device_bytes=lib.g2s_device_pool_bytes(out), reads=p.n_reads,
                    bases=p.base_off[p.n_reads], held_on_device=held["held_on_device"],
                    bases_bytes_to_host=held["bases_bytes_to_host"], **{k: v for k, v in P.test_last_dpool().items() if k.startswith("text")})
        lib.g2s_device_pool_free(out)
        finish(h, t, laps, sets)
        laps["whole"] = (time.perf_counter() - t0) * 1e3
        return laps, info

    sets = []
    run_pool(sets)      # (the process's first calls: HIP's start-up, left out)
    _, info = run_dpool(sets)
    rows = {"pool": [], "dpool": []}
    for _ in range(a.calls):
        rows["pool"].append(run_pool())
        rows["dpool"].append(run_dpool()[0])
    out = dict(workload="readfilter_handover", pairs=a.pairs, gaps=n, k=a.k, calls=a.calls, threads=a.threads,
               bam_mb=round(len(bam) / 1e6, 1), same_sets=sets[0] == sets[1], kmers=sets[0][0], pool_info=info,
               text=P.last_filter_text(), build_on_device=P.test_last_pool_build()["on_device"])
    for leg, calls in rows.items():
        out[leg] = {lap: dict(min=round(min(c[lap] for c in calls), 1), max=round(max(c[lap] for c in calls), 1),
                              mean=round(sum(c[lap] for c in calls) / len(calls), 1)) for lap in calls[0]}
        out[leg + "_whole_ms"] = [round(c["whole"], 1) for c in calls]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--gaps", type=int, default=1000)
    ap.add_argument("--loop-gaps", type=int, default=20)
    ap.add_argument("--scaffolds", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--host-inflate", action="store_true", help="add a leg with G2S_HOST_INFLATE=1")
    ap.add_argument("--one-pass", action="store_true", help="ask for one-pass mode (g2s_filter_set_one_pass(1))")
    ap.add_argument("--resident-cap", type=int, default=None, help="G2S_FILTER_RESIDENT_CAP for the legs")
    ap.add_argument("--store", choices=("0", "1"), default=None, help="G2S_FILTER_STORE for the legs")
    ap.add_argument("--handover", action="store_true", help="time the hand-over of the reads to the set build, two ways")
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--k", type=int, default=31)
    a = ap.parse_args()
    if a.resident_cap is not None:
        os.environ["G2S_FILTER_RESIDENT_CAP"] = str(a.resident_cap)
    if a.store is not None:
        os.environ["G2S_FILTER_STORE"] = a.store
    if a.one_pass:
        P.filter_set_one_pass(1)
    t0 = time.time()
    scaffold_len = max(10000, a.pairs // a.scaffolds * 2)
    refs, recs, _ = BW.simulate_library(a.seed, n_scaffolds=a.scaffolds, scaffold_len=scaffold_len,
                                        gap=(scaffold_len // 2, 300), pairs=a.pairs // a.scaffolds, mean=300, sd=20,
                                        unmapped_pairs=a.pairs // 100, ambiguous=0.0)
    bam = BW.bam_bytes(refs, recs)
    shuffled = None
    if not a.handover:
        recs = list(recs)
        random.Random(a.seed + 1).shuffle(recs)
        shuffled = BW.bam_bytes(refs, recs)
    del recs
    t_sim = time.time() - t0
    rng = random.Random(a.seed)
    gaps = [(rng.choice(refs)[0], rng.randrange(1000, scaffold_len - 1000), rng.randrange(50, 500), rng.randrange(30, 100))
            for _ in range(a.gaps)]
    mean, sd = 300, 20
    if a.handover:
        return handover(a, bam, gaps, mean, sd)
    # the per-gap loop on the first gaps
    t0 = time.perf_counter()
    loop = []
    for s, bp, gl, fl in gaps[:a.loop_gaps]:
        loop.append(P.filter_reads(bam, mean=mean, std_dev=sd, scaffold=s, breakpoint=bp, gap_length=gl, flank_length=fl,
                                   threads=a.threads))
    t_loop = time.perf_counter() - t0
    out = dict(workload="readfilter_gaps", pairs=a.pairs, records=loop[0][4] if loop else None, gaps=a.gaps,
               bam_mb=round(len(bam) / 1e6, 1), simulate_s=round(t_sim, 1),
               per_gap_s_measured=round(t_loop, 3), per_gap_gaps_measured=a.loop_gaps,
               per_gap_s_extrapolated=round(t_loop / max(1, a.loop_gaps) * a.gaps, 2))
    runs = [("host", bam, -1), ("device_first", bam, a.device), ("device", bam, a.device)]
    if a.host_inflate:
        runs.append(("device_host_inflate", bam, a.device))
    runs += [("shuffled_host", shuffled, -1), ("shuffled_device", shuffled, a.device)]
    # (the shuffled file's reads come out in its own order: checked against the per-gap filter on that file)
    check = {id(bam): loop, id(shuffled): [P.filter_reads(shuffled, mean=mean, std_dev=sd, scaffold=s, breakpoint=bp,
                                                          gap_length=gl, flank_length=fl) for s, bp, gl, fl in gaps[:3]]}
    for label, data, dev in runs:
        if label == "device_host_inflate":
            os.environ["G2S_HOST_INFLATE"] = "1"
        t0 = time.perf_counter()
        got, st = P.filter_reads_gaps(data, mean, sd, gaps, device=dev, threads=a.threads)
        dt = time.perf_counter() - t0
        os.environ.pop("G2S_HOST_INFLATE", None)
        inf, txt = P.last_filter_inflate(), P.last_filter_text()
        want = check[id(data)]
        assert got[:len(want)] == want, label + ": differs from the per-gap filter"
        out[label] = dict(s=round(dt, 3), inflate_ms=round(st["ms_inflate"], 1), join_ms=round(st["ms_join"], 1),
                          text_ms=round(st["ms_text"], 1), on_device=st["on_device"], file_passes=st["file_passes"],
                          text_on_device=txt["one_pass"], text_reason=P.TEXT_REASONS[txt["reason"]],
                          resident_mb=round(txt["resident_bytes"] / 1e6, 1), store=P.last_filter_store(),
                          extracted=sum(x[3] for x in got), inflate_on_device=inf["on_device"],
                          refill_a_ms=round(inf["ms_pass_a_inflate"], 1), refill_b_ms=round(inf["ms_pass_b_inflate"], 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
