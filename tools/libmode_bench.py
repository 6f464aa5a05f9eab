"""Libraries mode (Gap2Seq.py -l: one read set per gap) in one process: a set graph (Graph.from_sets) and one
g2s_fill_sets list against the same gaps done one by one in process (Graph.from_seqs + Session.execute_single per
gap, what the wrapper's per-gap Gap2Seq-core runs do minus the process start).  Synthetic workload: a
cases.toy_genome genome, cases.cut_gaps gaps, per gap the reads of a window around the gap plus a window from
elsewhere (the sets overlap).  Prints one JSON line.

    python tools/libmode_bench.py [--gaps 1000,10000] [--loop-gaps 200] [--k 31]

With --shared-bases N the workload gets a list of N bases of reads that a share --flagged F of the sets hold behind
their own (the libraries flow's unmapped reads), and the set graph is built both ways: Graph.from_sets on the expanded
lists and Graph.from_pool on the pool (--build sets|pool|both; one way a process keeps the peak resident sizes apart).
Per way: build_ms (the best and all of --reps), fill_ms, what g2s_test_last_pool_build counted, and the process's
peak resident size (resource.getrusage, MB) before the lists were made, before the build and after the fill.

    python tools/libmode_bench.py --gaps 1000 --shared-bases 2000000 --flagged 0.1 [--build pool] [--reps 3]
"""
import argparse
import json
import os
import resource
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
    res, tm = s.fill_sets(gaps, list(range(len(gaps))), want_timing=True)
    t3 = time.perf_counter()
    filled = sum(r.count > 0 for r in res)
    s.destroy()
    g.free()
    return dict(build_ms=(t1 - t0) * 1e3, session_ms=(t2 - t1) * 1e3, fill_ms=(t3 - t2) * 1e3,
                resident_launches=tm.resident_launches, resident_fallbacks=tm.resident_fallbacks,
                host_finished_gaps=tm.host_finished_gaps, gaps_per_s=len(gaps) / (t3 - t0), filled=filled)


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


def peak_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def shared_workload(n, k, shared_bases, flagged, seed=3):
    """workload(n, k) as a pool: (seqs, set_lists, shared, set_shared, gaps); the shared list is reads of 150 random
    bases, every round(1 / flagged)-th set holds it"""
    sets, gaps = workload(n, k, seed)
    seqs, set_lists = [], []
    for reads in sets:
        set_lists.append(list(range(len(seqs), len(seqs) + len(reads))))
        seqs.extend(reads)
    rng = cases.SplitMix(seed + 77)
    shared = []
    for _ in range(shared_bases // 150):
        shared.append(len(seqs))
        seqs.append(cases.random_dna(rng, 150))
    nflag = int(round(flagged * n))
    step = n / nflag if nflag else 0
    marks = {int(i * step) for i in range(nflag)}
    return seqs, set_lists, shared, [1 if s in marks else 0 for s in range(n)], gaps


def run_shared(way, seqs, set_lists, shared, set_shared, gaps, k, reps):
    out = {"peak_mb_start": peak_mb()}
    if way == "sets":
        sets = [[seqs[i] for i in own] + ([seqs[i] for i in shared] if set_shared[s] else []) for s, own in enumerate(set_lists)]
        build = lambda: P.Graph.from_sets(sets, k, 1)  # noqa: E731
    else:
        build = lambda: P.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared)  # noqa: E731
    out["peak_mb_lists"] = peak_mb()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g = build()
        times.append((time.perf_counter() - t0) * 1e3)
        if len(times) < reps:
            g.free()
    if way == "pool":
        out["pool_build"] = P.test_last_pool_build()
    s = P.Session(g, 0, d_err=500, randseed=1)
    t0 = time.perf_counter()
    res, tm = s.fill_sets(gaps, list(range(len(gaps))), want_timing=True)
    out.update(build_ms=min(times), build_ms_all=[round(t, 1) for t in times], fill_ms=(time.perf_counter() - t0) * 1e3,
               resident_launches=tm.resident_launches, resident_fallbacks=tm.resident_fallbacks,
               host_finished_gaps=tm.host_finished_gaps, filled=sum(r.count > 0 for r in res), kmers=g.num_kmers, peak_mb_end=peak_mb())
    s.destroy()
    g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", default="1000,10000")
    ap.add_argument("--loop-gaps", type=int, default=200, help="gaps of each list the per-gap loop is timed on")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--shared-bases", type=int, default=None, help="bases of the list the flagged sets share (0: none)")
    ap.add_argument("--flagged", type=float, default=0.1, help="share of the sets that hold the shared list")
    ap.add_argument("--build", choices=["sets", "pool", "both"], default="both")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if P.G2S.device_count() < 1:
        raise SystemExit("libmode_bench: no gfx950 device")
    out = {"k": a.k}
    warm = workload(16, a.k, seed=9)
    run_sets(*warm, a.k)
    if a.shared_bases is not None:
        out.update(shared_bases=a.shared_bases, flagged=a.flagged)
        for n in [int(x) for x in a.gaps.split(",")]:
            w = shared_workload(n, a.k, a.shared_bases, a.flagged)
            for way in (["pool", "sets"] if a.build == "both" else [a.build]):
                out["%s_%d" % (way, n)] = run_shared(way, *w, a.k, a.reps)
        print(json.dumps(out))
        return
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
