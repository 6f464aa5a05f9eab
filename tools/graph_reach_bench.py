#!/usr/bin/env python3
"""File to uploaded graph with and without reach records ("A graph bounded to its gap list's reach").

For each config the reads go to a FASTA file and the gaps to a scaffolds file; what is timed is
Graph.from_files(...) + upload(0) — for the three reach modes with g2s_scaffolds_reach inside the timed region, as
Gap2Seq-core does it.  Variants: plain (g2s_graph_build_files), never, auto, always, and — with --parent LIB, another
build's libg2s_hip.so, e.g. the parent commit's — that library's plain call.

Protocol: a fresh process per library and round, the two libraries alternating; inside a process a warm-up build first
(HIP's start-up and the first load of the kernels stay out), then two repetitions of all modes, the order rotated by
the round in the first and reversed in the second, so that no mode always runs behind the same one.  Every time is
printed and appended to --out as a JSON line; the summary gives mean [min-max] per variant.

    python tools/graph_reach_bench.py --configs C2,C5,C4 --rounds 3 --parent /path/to/parent/libg2s_hip.so
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: genome bp, k, gaps, min_len, max_len, d_err (bench.py's configs; C4 with the 10 000 gaps the comparison asks for)
CONFIGS = {
    "C2": (3000000, 31, 500, 200, 1000, 500),
    "C4": (60000000, 63, 10000, 200, 1000, 500),
    "C5": (3000000, 31, 1000, 2000, 5000, 2000),
}
FUZ = 10
WARM = "ACGTTGCATTGACCAGTAGGACCATTTGACAAGGATTTACCAGGGATACAGGACAGATTTAGAC" * 3
MODES = ["plain", "never", "auto", "always"]


def worker_parent(lib_path, reads, k):
    """another build's library: its plain call through bare ctypes (it may lack the newer symbols)"""
    lib = C.CDLL(lib_path)
    lib.g2s_graph_num_kmers.restype = C.c_uint64
    lib.g2s_graph_num_kmers.argtypes = [C.c_void_p]
    lib.g2s_graph_free.argtypes = [C.c_void_p]
    lib.g2s_graph_upload.argtypes = [C.c_void_p, C.c_int]

    def build(path, kk):
        h = C.c_void_p()
        assert lib.g2s_graph_build_files(path.encode(), kk, 1, 0, C.byref(h)) == 0
        assert lib.g2s_graph_upload(h, 0) == 0
        return h
    warm = reads + ".warm.fa"
    with open(warm, "w") as f:
        f.write(">w\n" + WARM + "\n")
    lib.g2s_graph_free(build(warm, 31))
    out = []
    for _ in range(2):
        t0 = time.perf_counter()
        h = build(reads, k)
        out.append(dict(mode="parent_plain", s=time.perf_counter() - t0, kmers=lib.g2s_graph_num_kmers(h)))
        lib.g2s_graph_free(h)
    return out


def worker_new(reads, scaf, k, d_err, rnd):
    from gap2seq_amd import lib as P
    g = P.Graph.from_seqs([WARM], 31, 1)
    g.upload(0)
    g.free()
    text = open(scaf).read()
    first = MODES[rnd % len(MODES):] + MODES[:rnd % len(MODES)]
    out = []
    for order in (first, first[::-1]):
        for mode in order:
            t0 = time.perf_counter()
            if mode == "plain":
                g = P.Graph.from_files(reads, k, 1)
            else:
                recs = P.scaffolds_reach(text, k, FUZ, d_err)
                g = P.Graph.from_files(reads, k, 1, reach=recs,
                                       reach_mode=dict(never=P.REACH_NEVER, auto=P.REACH_AUTO, always=P.REACH_ALWAYS)[mode])
            g.upload(0)
            rec = dict(mode=mode, s=time.perf_counter() - t0, kmers=g.num_kmers)
            if mode == "always":
                rec.update(P.test_last_graph_reach())
            g.free()
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="graph_reach_bench.jsonl")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--worker", nargs="*", default=None)
    a = ap.parse_args()
    if a.worker is not None:
        which, reads, scaf, k, d_err, rnd = a.worker
        res = worker_parent(a.parent, reads, int(k)) if which == "parent" else worker_new(reads, scaf, int(k), int(d_err), int(rnd))
        print(json.dumps(res))
        return 0
    from gap2seq_amd import lib as P
    for name in a.configs.split(","):
        bp, k, ngaps, lo, hi, d_err = CONFIGS[name]
        reads = P.G2S.synth_genome(bp, 3, 20240101)
        scaf = P.G2S.synth_gaps(reads, k, FUZ, ngaps, lo, hi, 20240103)
        rp, sp = os.path.join(a.tmp, "reach_%s.fa" % name), os.path.join(a.tmp, "reach_%s_scaf.fa" % name)
        with open(rp, "w") as f:
            f.write(reads)
        with open(sp, "w") as f:
            f.write(scaf)
        del reads, scaf
        times, last = {}, {}
        for rnd in range(a.rounds):
            for which in (["parent"] if a.parent else []) + ["new"]:
                cmd = [sys.executable, os.path.abspath(__file__), "--parent", a.parent, "--worker", which, rp, sp, str(k), str(d_err), str(rnd)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    return 1
                for rec in json.loads(r.stdout.strip().splitlines()[-1]):
                    rec.update(config=name, round=rnd)
                    times.setdefault(rec["mode"], []).append(rec["s"])
                    last[rec["mode"]] = rec
                    line = json.dumps(rec)
                    print(line, flush=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        for mode, ts in times.items():
            extra = ""
            if mode == "always":
                r = last[mode]
                extra = "  kept %d of %d, %d levels, search %.1f ms = %.2f us a level, %d regrowths" % (
                    r["kept_kmers"], r["full_kmers"], r["levels"], r["ms_search"], 1e3 * r["ms_search"] / max(1, r["levels"]), r["regrowths"])
            line = "SUMMARY %s %-12s %.4f [%.4f-%.4f] n=%d%s" % (name, mode, sum(ts) / len(ts), min(ts), max(ts), len(ts), extra)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(dict(summary=line)) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
