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

Every batched run carries the store route's hook (g2s_test_last_filter_store: used, records, store_bytes, store_cap,
rows_cap, device_bytes, overflow) under "store".  Every run also carries the reader's own laps (g2s_test_last_filter_inflate): whether the file was inflated on the
device and the time inside the reader's refills in pass A and pass B.

Prints one JSON line.  The library is tests/bamwriter.simulate_library's, about --pairs read pairs on 10 scaffolds,
with --gaps gaps at random breakpoints; the same gaps for all three, on the coordinate-sorted file and on the same
records shuffled (where the host joins sort their index, which a sorted file spares them).

  python tools/readfilter_bench.py [--pairs 1000000] [--gaps 1000] [--loop-gaps 20] [--device 0] [--threads 0]
                                   [--host-inflate] [--one-pass] [--resident-cap BYTES] [--store 0|1]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bamwriter as BW  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402


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
    recs = list(recs)
    random.Random(a.seed + 1).shuffle(recs)
    shuffled = BW.bam_bytes(refs, recs)
    del recs
    t_sim = time.time() - t0
    rng = random.Random(a.seed)
    gaps = [(rng.choice(refs)[0], rng.randrange(1000, scaffold_len - 1000), rng.randrange(50, 500), rng.randrange(30, 100))
            for _ in range(a.gaps)]
    mean, sd = 300, 20
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
