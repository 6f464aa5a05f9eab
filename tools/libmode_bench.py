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

With --reach (pool builds) every set gets a reach record — its gap, with the sound radius reach_radius(gap, 500) —
through Graph.from_pool(..., reach=...), and the line also holds what g2s_test_last_pool_reach counted: the k-mers
kept, and the k-mers of the full sets where the build counted them (the host build; null on the device).  --model
prints instead, without a device, the k-mers the brute-force model of tests/reach_cases.py keeps for the same workload
(and the full sets' k-mers): the number the graph's k-mer count with --reach must equal.
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


def model_kmers(seqs, set_lists, shared, set_shared, gaps, k):
    """(kept, full) summed over the sets, by the model of tests/reach_cases.py on two count tables (the shared list
    counted once)"""
    import reach_cases as RC
    sh = RC.kmer_counts([seqs[i] for i in shared], k)
    kept_all = full_all = 0
    for s, own_list in enumerate(set_lists):
        own = RC.kmer_counts([seqs[i] for i in own_list], k)
        flagged = bool(set_shared[s])
        member = (lambda x: x in own or x in sh) if flagged else (lambda x: x in own)  # (solid = 1)
        full_all += len(own) + (sum(1 for x in sh if x not in own) if flagged else 0)
        g = gaps[s]
        gd = dict(left=g.left, right=g.right, gap_len=g.gap_len, lmf=g.lmf, rmf=g.rmf)
        kept = {x for x in RC.seeds_of(gd, k) if member(x)}
        frontier, level, radius = list(kept), 0, P.reach_radius(g, 500)
        while frontier and level < radius:
            nxt = []
            for x in frontier:
                for y in RC.neighbours(x):
                    if y not in kept and member(y):
                        kept.add(y)
                        nxt.append(y)
            frontier, level = nxt, level + 1
        kept_all += len(kept)
    return kept_all, full_all


def run_shared(way, seqs, set_lists, shared, set_shared, gaps, k, reps, reach=False):
    out = {"peak_mb_start": peak_mb()}
    if way == "sets":
        sets = [[seqs[i] for i in own] + ([seqs[i] for i in shared] if set_shared[s] else []) for s, own in enumerate(set_lists)]
        build = lambda: P.Graph.from_sets(sets, k, 1)  # noqa: E731
    elif reach:
        records = [(g, P.reach_radius(g, 500)) for g in gaps]
        build = lambda: P.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared, reach=records)  # noqa: E731
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
    if way == "pool" and reach:
        out["pool_reach"] = P.test_last_pool_reach()
    t0 = time.perf_counter()
    s = P.Session(g, 0, d_err=500, randseed=1)
    out["session_ms"] = (time.perf_counter() - t0) * 1e3
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
    ap.add_argument("--reach", action="store_true", help="pool builds with a reach record a set (the sound radius)")
    ap.add_argument("--model", action="store_true", help="no device: the k-mers the model keeps for the --reach workload")
    a = ap.parse_args()
    if a.model:
        out = {"k": a.k, "shared_bases": a.shared_bases, "flagged": a.flagged}
        for n in [int(x) for x in a.gaps.split(",")]:
            kept, full = model_kmers(*shared_workload(n, a.k, a.shared_bases or 0, a.flagged), a.k)
            out["model_%d" % n] = dict(kept_kmers=kept, full_kmers=full)
        print(json.dumps(out))
        return
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
                out["%s_%d" % (way, n)] = run_shared(way, *w, a.k, a.reps, reach=a.reach and way == "pool")
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
