"""tests/d2_witness.py — which phase D2 kernel took which gap of a list, from the library's own log (G2S_D2_LOG, one
row per closure a g2s_d2_* workgroup took: tools/d2_log.py).  The switch that turns the log on is read once per
process, so the list runs in a child process; shared by tests/test_gpu_edges.py (the planted ladders) and
tests/test_gpu_d2_designed.py (the designed components)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_D2_CHILD = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1]), os.path.join(sys.argv[1], "tests")]
import cases
from gap2seq_amd import lib as P
P.load_library()
what = json.loads(sys.argv[2])
if "designs" in what:
    import d2_cases
    seqs, gaps, idx, _ = d2_cases.design_list(what["designs"], pad=100)
    d_err = what["designs"]
elif "trace" in what:  # (tests/trace_cases.py: the first copy of every planted gap of one list)
    import trace_cases
    seqs, gaps, idx = trace_cases.trace_list(what["trace"])
    idx = [v[0] for v in idx.values()]
    d_err = what["d_err"]
else:
    seqs, gaps, idx = cases.edge_ladder_list(what["ladders"], pad=100)
    d_err = 10
pg = P.Graph.from_seqs(seqs, 31, 1)
sess = P.Session(pg, 0, d_err=d_err, randseed=5)
res, tm = sess.fill_batch([P.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"]) for g in gaps], True)
sess.destroy()
pg.free()
out = dict(idx=idx, watchdog=tm.watchdog_gaps, resident=tm.resident_launches, fallbacks=tm.resident_fallbacks)
if "designs" in what:  # every field of every result, for the comparison with the oracle in the parent
    out["host_finished"] = tm.host_finished_gaps
    out["results"] = [[r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, list(r.substats), r.phaseC_count, list(r.lengths)] for r in res]
print(json.dumps(out))
"""
FIELDS = ("count", "left_fuz", "right_fuz", "flags", "draws", "fill", "substats", "phaseC_count", "lengths")


def _run_logged(tmp_path, what, names, timeout, env):
    log = tmp_path / ("d2_%s.log" % "_".join("%s%s" % kv for kv in sorted(env.items())))
    env = dict(os.environ, G2S_DEVICE_D2="1", G2S_D2_PROF="1", G2S_D2_LOG=str(log), G2S_RESIDENT="1", G2S_D2_SMALL_WAVES="1",
               **env)
    out = subprocess.run([sys.executable, "-c", _D2_CHILD, ROOT, json.dumps(what)], env=env, capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["watchdog"] == 0 and r["resident"] == 1 and r["fallbacks"] == 0
    rows = {}
    for line in open(log):
        w = line.split()
        if len(w) == 16:
            w = [int(x) for x in w]
            rows.setdefault(w[0] & 0xFFFFFFFF, []).append(dict(
                kernel=w[15] & 1, rc=(w[2] >> 32) & 0xFFFF, nrec=w[0] >> 32, ns=w[1] & 0xFFFFFFFF, nv=(w[1] >> 32) & 0xFFFF,
                ne=w[2] & 0xFFFFFFFF))
    return {name: rows.get(i, []) for i, name in zip(r["idx"], names)}, r


def _d2_log(tmp_path, names, **env):
    """{planted gap name: [dict(kernel=0 small | 1 big, rc=0 taken | passed on, ...)]} from G2S_D2_LOG (written when the
    session ends; in a child process, as the switch that turns the log on is read once per process).  The list is
    finished on the device with phase D2 there (G2S_DEVICE_D2=1); g2s_d2_small runs on one wave a closure, so that
    the log's workgroup-size bit tells the two instantiations apart."""
    return _run_logged(tmp_path, dict(ladders=names), names, 300, env)[0]


def d2_log_of_designs(tmp_path, d_err, **env):
    """The same for the list of tests/d2_cases.py's designs of one -dist-error: {design: [dict(kernel, rc, nrec, ns (closure
    segments on paths to a sink), nv, ne (nodes and edges of the run graph; 0 where the closure went through as a
    DAG or was passed on before they were counted))] in the order small, large}, the list's results as the objects
    tests/test_gpu_parity.py compares with the oracle, and the call's timing counters."""
    import types
    import d2_cases
    by, r = _run_logged(tmp_path, dict(designs=d_err), d2_cases.names_at(d_err), 120, env)
    res = [types.SimpleNamespace(**dict(zip(FIELDS, x))) for x in r["results"]]
    tm = types.SimpleNamespace(watchdog_gaps=r["watchdog"], resident_launches=r["resident"], resident_fallbacks=r["fallbacks"],
                               host_finished_gaps=r["host_finished"])
    return by, res, tm
