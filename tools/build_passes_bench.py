#!/usr/bin/env python3
"""Time the solid-set stage of the single-graph build on bench.py's read sets: the one-sort device count, the key-range
pass form (gap2seq_amd/csrc/solid_passes.h) forced to a number of passes with G2S_BUILD_PASS_KEYS, and the host count
(G2S_HOST_BUILD=1).  The time is the build's own G2S_DEBUG line ("solid k-mer set %.3f s"); the ways are interleaved,
--reps builds each, and the median and the spread of each are printed as one JSON line.

  python tools/build_passes_bench.py --config C4 --reps 5 --passes 2,4,8 --threads 16
  python tools/build_passes_bench.py --config C4 --once 4        # one one-sort and one 4-pass build (for a kernel trace)
  python tools/build_passes_bench.py --config C4 --k 31 --copies 36 --no-sort --no-host --reps 1   # 2^32 positions and more

Needs a GPU; nothing here falls back to the host."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402

LINE = re.compile(r"graph build: (\d+) k-mers; solid k-mer set ([0-9.]+) s \(([^)]*)\), tables \+ unitig order ([0-9.]+) s")
VALID = re.compile(r"(\d+) of (\d+) positions valid")
SWITCHES = ("G2S_HOST_BUILD", "G2S_BUILD_PASS_KEYS")


def build(seqs, k, solid, threads, env):
    """one build with G2S_DEBUG's lines caught: dict(kmers, set_s, how, tables_s, wall_s, info, stderr)"""
    for name in SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(env)
    os.environ["G2S_DEBUG"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            g = P.Graph.from_seqs(seqs, k, solid, threads)
            wall = time.perf_counter() - t0
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    info = P.test_last_solid_count()
    n = g.num_kmers
    g.free()
    for name in SWITCHES:
        os.environ.pop(name, None)
    m = LINE.search(text)
    if not m:
        raise SystemExit("no build line on stderr:\n" + text)
    return dict(kmers=n, set_s=float(m.group(2)), how=m.group(3), tables_s=float(m.group(4)), wall_s=wall, info=info, stderr=text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", default="2,4,8")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--k", type=int, default=0, help="k-mer length (default: the config's)")
    ap.add_argument("--copies", type=int, default=1, help="the read set this many times (the same memory, listed again)")
    ap.add_argument("--once", type=int, default=0, help="one one-sort build and one build of this many passes, nothing else")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-sort", action="store_true",
                    help="a text beyond one sort: no switch set means the pass form at the library's own pass size (way 'auto')")
    args = ap.parse_args()
    genome_bp, k = bench.CONFIGS[args.config][:2]
    k = args.k or k
    reads = P.G2S.synth_genome(genome_bp, 3, bench.GENOME_SEED)
    seqs = [ln.encode("ascii") for ln in reads.splitlines() if not ln.startswith(">")]
    del reads
    seqs = seqs * args.copies
    positions = sum(len(s) + 1 for s in seqs)

    # the valid keys, from a build in one forced pass (also the warm-up of the pass form's code)
    # (a text beyond one sort takes the pass form by itself, at the library's own pass size)
    first = build(seqs, k, 1, args.threads, {} if args.no_sort else {"G2S_BUILD_PASS_KEYS": str(positions)})
    m = VALID.search(first["stderr"])
    if not m:
        raise SystemExit("the pass form did not run on a device:\n" + first["stderr"])
    valid = int(m.group(1))
    ways = {"auto": {}} if args.no_sort else {"one-sort": {}}
    for p in ([args.once] if args.once else [int(x) for x in args.passes.split(",") if x]):
        ways["passes-%d" % p] = {"G2S_BUILD_PASS_KEYS": str(-(-valid // p) + valid // (64 * p))}  # (bins do not cut evenly)
    if not args.once and not args.no_host:
        ways["host"] = {"G2S_HOST_BUILD": "1"}
    runs = {w: [] for w in ways}
    if not args.no_sort:
        build(seqs, k, 1, args.threads, {})  # warm-up of the one-sort way
    for rep in range(1 if args.once else args.reps):
        for w, env in ways.items():
            r = build(seqs, k, 1, args.threads, env)
            r.pop("stderr")
            runs[w].append(r)
            print("rep %d %-9s set %.3f s tables %.3f s wall %.3f s (%s) %d k-mers, %d passes, largest %d" % (
                rep, w, r["set_s"], r["tables_s"], r["wall_s"], r["how"], r["kmers"], r["info"]["passes"],
                r["info"]["max_pass_keys"]), flush=True)
    out = {"config": args.config, "k": k, "positions": positions, "valid_keys": valid, "copies": args.copies, "ways": {}}
    for w, rs in runs.items():
        ts = sorted(r["set_s"] for r in rs)
        out["ways"][w] = dict(median_s=statistics.median(ts), min_s=ts[0], max_s=ts[-1], reps=len(ts), kmers=rs[0]["kmers"],
                              passes=rs[0]["info"]["passes"], on_device=rs[0]["info"]["on_device"])
    kmers = {v["kmers"] for v in out["ways"].values()} | {first["kmers"]}
    out["same_kmers"] = len(kmers) == 1
    print(json.dumps(out))
    return 0 if out["same_kmers"] else 1


if __name__ == "__main__":
    sys.exit(main())
