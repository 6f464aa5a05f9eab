"""GPU box: K consecutive lists over a team of N sessions (g2s_session_set_team, one share per session) through
g2s_fill_begin / g2s_fill_end with 1, 2 and 3 lists in flight, the team's lists queued at g2s_fill_begin
(G2S_TEAM_IN_FLIGHT unset) and kept back for g2s_fill_end (=0), alternating in one process — ms per list, and whether
every list's results are the same in every setting.  The sessions share device 0 unless devices are named: one device
standing in for N shows that the scheduling works and what it costs, not what N GPUs gain.
usage: team_stream_probe.py [NSESSIONS] [NGAPS] [KLISTS] [DEVICE ...]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B
from gap2seq_amd import lib as P

nsess = int(sys.argv[1]) if len(sys.argv) > 1 else 2
ngaps = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
klists = int(sys.argv[3]) if len(sys.argv) > 3 else 6
devices = [int(x) for x in sys.argv[4:]] or [0]
reps = 7
reads = P.G2S.synth_genome(3000000, 3, B.GENOME_SEED)
seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
gaps = B.parse_gaps(P.G2S.synth_gaps(reads, 31, 10, ngaps, 200, 1000, B.GAP_SEED), 10)
graph = P.Graph.from_seqs(seqs, 31, 1)
team = [P.Session(graph, devices[t % len(devices)], d_err=500, randseed=1) for t in range(nsess)]
lead = team[0]
lead.set_team(team[1:], P.G2S_GROUP_PER_SESSION)
lib = P.load_library()
arr, keep = P._gap_array([P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]) for g in gaps])
n = len(gaps)
nbytes = lib.g2s_team_arena_bytes(lead.h, arr, n)
bufs = []
for _ in range(klists):  # (every list has buffers of its own: up to three are written at a time)
    arena, rbuf = P.HostBuffer(nbytes), P.HostBuffer(C.sizeof(P.g2s_result) * n)
    bufs.append((arena, rbuf, rbuf.array(P.g2s_result, n), C.cast(arena.p, C.c_void_p)))


def run(depth, switch):
    """the K lists, `depth` in flight; returns (seconds, most lists launched at a g2s_fill_begin's return)"""
    if switch:
        os.environ.pop("G2S_TEAM_IN_FLIGHT", None)
    else:
        os.environ["G2S_TEAM_IN_FLIGHT"] = "0"
    lead.srand(1)
    launched = 0
    t0 = time.perf_counter()
    for arena, rbuf, res, ap in bufs:
        if lib.g2s_fill_in_flight(lead.h) == depth:
            P._check(lib.g2s_fill_end(lead.h))
        P._check(lib.g2s_fill_begin(lead.h, arr, n, res, ap, nbytes))
        launched = max(launched, lib.g2s_fill_in_flight_launched(lead.h))
    while lib.g2s_fill_in_flight(lead.h) > 0:
        P._check(lib.g2s_fill_end(lead.h))
    return time.perf_counter() - t0, launched


def keys():
    out = []
    for arena, rbuf, res, ap in bufs:
        raw = arena.raw
        out.append([(r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, raw[r.fill_off:r.fill_off + max(0, r.fill_len)]) for r in (res[i] for i in range(n))])
    return out


settings = [(depth, switch) for depth in (1, 2, 3) for switch in (True, False)]
times = {st: [] for st in settings}
launched = {}
want = None
same = True
try:
    for st in settings:  # (warm-up: twins, buffers, the first lists' allocations)
        run(*st)
    for rep in range(reps):
        for st in settings:  # (alternating: every setting sees the same drift of the box)
            t, launched[st] = run(*st)
            times[st].append(t)
            if rep == 0:
                got = keys()
                if want is None:
                    want = got
                same = same and got == want
    tm = lead.last_timing()
    print("team of %d sessions on device(s) %s, %d lists of %d gaps; the last list: sharded %d, groups %d, fallbacks %d"
          % (nsess, devices, klists, n, tm.team_d3_sharded, tm.team_groups, tm.resident_fallbacks))
    for depth, switch in settings:
        ts = sorted(times[(depth, switch)])
        print("in flight %d, team lists queued at begin %-3s (launched at most %d): best %.3f ms per list, median %.3f, worst %.3f; %.2f M gaps/s at best"
              % (depth, "yes" if switch else "no", launched[(depth, switch)], ts[0] / klists * 1e3, ts[len(ts) // 2] / klists * 1e3,
                 ts[-1] / klists * 1e3, n * klists / ts[0] / 1e6))
    print("every list's results identical in every setting: %s" % same)
finally:
    os.environ.pop("G2S_TEAM_IN_FLIGHT", None)
    while lib.g2s_fill_in_flight(lead.h) > 0:
        lib.g2s_fill_end(lead.h)
    for s in team:
        s.destroy()
    for arena, rbuf, res, ap in bufs:
        arena.free()
        rbuf.free()
    graph.free()
sys.exit(0 if same else 1)
