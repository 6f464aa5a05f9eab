"""Libraries mode (Gap2Seq.py -l: one read set per gap) in one process: a set graph (Graph.from_sets) and one
g2s_fill_sets list against the same gaps done one by one in process (Graph.from_seqs + Session.execute_single per
gap, what the wrapper's per-gap Gap2Seq-core runs do minus the process start).  Synthetic workload: a
cases.toy_genome genome, cases.cut_gaps gaps, per gap the reads of a window around the gap plus a window from
elsewhere (the sets overlap).  Prints one JSON line.

    python tools/libmode_bench.py [--gaps 1000,10000] [--loop-gaps 200] [--k 31]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402


def workload(n, k, seed=3):
    genome = cases.toy_genome(seed, max(200000, 40 * n), k, repeats=20, snp_every=0)[0]
    rng = cases.SplitMix(seed)
    raw = cases.cut_gaps(seed, genome, k, 10, n, 20, 300, 500)
    sets, gaps = [], []
    for g in raw:
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 300), min(len(genome), pos + g["true_len"] + 300)
        o = rng.randint(0, len(genome) - 500)
        sets.append([genome[lo:hi], genome[lo + 50:hi - 50], genome[o:o + 500]])
        gaps.append(P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]))
    return sets, gaps


def run_sets(sets, gaps, k):
    t0 = time.perf_counter()
    g = P.Graph.from_sets(sets, k, 1)
    t1 = time.perf_counter()
    s = P.Session(g, 0, d_err=500, randseed=1)
    t2 = time.perf_counter()
    res = s.fill_sets(gaps, list(range(len(gaps))))
    t3 = time.perf_counter()
    filled = sum(r.count > 0 for r in res)
    s.destroy()
    g.free()
    return dict(build_ms=(t1 - t0) * 1e3, session_ms=(t2 - t1) * 1e3, fill_ms=(t3 - t2) * 1e3,
                gaps_per_s=len(gaps) / (t3 - t0), filled=filled)


def run_loop(sets, gaps, k):
    t0 = time.perf_counter()
    filled = 0
    for seqs, gp in zip(sets, gaps):
        g = P.Graph.from_seqs(seqs, k, 1)
        s = P.Session(g, 0, d_err=500, randseed=1)
        fa, _ = s.execute_single(gp.left, gp.right, gp.gap_len, k, solid=1, max_fuz=10)
        filled += "N" not in "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))
        s.destroy()
        g.free()
    dt = time.perf_counter() - t0
    return dict(gaps=len(gaps), ms=dt * 1e3, gaps_per_s=len(gaps) / dt, filled=filled)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", default="1000,10000")
    ap.add_argument("--loop-gaps", type=int, default=200, help="gaps of each list the per-gap loop is timed on")
    ap.add_argument("--k", type=int, default=31)
    a = ap.parse_args()
    if P.G2S.device_count() < 1:
        raise SystemExit("libmode_bench: no gfx950 device")
    out = {"k": a.k}
    warm = workload(16, a.k, seed=9)
    run_sets(*warm, a.k)
    for n in [int(x) for x in a.gaps.split(",")]:
        sets, gaps = workload(n, a.k)
        r = run_sets(sets, gaps, a.k)
        m = min(n, a.loop_gaps)
        lp = run_loop(sets[:m], gaps[:m], a.k)
        out["sets_%d" % n] = r
        out["loop_%d" % n] = lp
        out["speedup_%d" % n] = r["gaps_per_s"] / lp["gaps_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
