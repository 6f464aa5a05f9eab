#!/usr/bin/env python3
"""GPU box: one set list (g2s_fill_sets, 600 gaps of the kind tests/test_gpu_sets_resident.py fills, finished on the
device: phase D3 in its restart form) N times through one session; prints a digest of the first call's results (every
field and the fill text of every gap) and how many later calls differ from it.  With G2S_LIBRARY pointing at a
race-hunting build (gap2seq_amd/_jit, gap2seq_amd/_par — csrc/sync_debug.h) the digest has to be the normal build's.

  python tools/race_hunt_sets.py [N]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, SEED, D_ERR, FUZ, GAPS = 31, 7, 100, 10, 600


def workload():
    import cases
    hap = cases.toy_genome(41, 12000, K, repeats=6, tandem=2, snp_every=350)
    genome = hap[0]
    rng = cases.SplitMix(41 * 31 + K)
    sets, gaps, gap_set = [], [], []
    for i, g in enumerate(cases.cut_gaps(41, genome, K, FUZ, GAPS, 10, 160, D_ERR)):
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 150), min(len(genome), pos + g["true_len"] + 150)
        o = rng.randint(0, len(genome) - 400)
        reads = [h[lo:hi] for h in hap] + [genome[o:o + 400]]
        if i % 4 == 3:
            sets[-1].extend(reads)
        else:
            sets.append(reads)
        gaps.append(g)
        gap_set.append(len(sets) - 1)
    return sets, gaps, gap_set


def main():
    n_runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    from gap2seq_amd import lib as P
    sets, gaps, gap_set = workload()
    graph = P.Graph.from_sets(sets, K, 1)
    sess = P.Session(graph, 0, d_err=D_ERR, randseed=SEED)
    lst = [P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]) for g in gaps]

    def call():
        res, t = sess.fill_sets(lst, gap_set, want_timing=True)
        key = [(r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.substats, r.phaseC_count, r.lengths) for r in res]
        return hashlib.sha256(repr(key).encode()).hexdigest()[:20], res, t

    first, res, tm = call()
    bad, launches, fallbacks = 0, tm.resident_launches, tm.resident_fallbacks
    for _ in range(1, n_runs):
        d, _, t = call()
        bad += d != first
        launches = min(launches, t.resident_launches)
        fallbacks = max(fallbacks, t.resident_fallbacks)
    print(json.dumps({"library": os.path.basename(os.path.dirname(P.library_path())), "gaps": len(gaps), "runs": n_runs, "differ": bad,
                      "digest": first, "filled": sum(1 for r in res if r.count > 0), "resident_launches": launches,
                      "fallbacks": fallbacks, "draw_dependent": tm.draw_dependent_gaps, "host_finished": tm.host_finished_gaps,
                      "traced_in_fill": tm.traced_in_fill_gaps}))
    sess.destroy()
    graph.free()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
