"""Set lists finished on the device: g2s_fill_sets in resident mode (phase D3 in its restart form, d3_device.hip:
g2s_d3_restart — every gap reads the rand() stream from value 0).  Every comparison is exact equality of every result
field and the fill text; the references are the same list on the host path (G2S_RESIDENT=0) and the CPU oracle on a
graph of each gap's set alone."""
import json
import os
import subprocess
import sys

import pytest

import cases
import oracle_lib as O
import pool_cases as PC

pytestmark = pytest.mark.gpu

SEED = 7
D_ERR = 100
FUZ = 10


def _workload(k, seed, ngaps, solid=1, tandem=2, length=12000):
    """(sets, gaps, gap_set) as tests/test_gpu_sets.py builds them: per gap, reads of both haplotypes around the gap
    plus a window from elsewhere (sets overlap); every fourth gap shares the set of the gap in front of it; one gap
    names an empty set; one set is named by no gap."""
    hap = cases.toy_genome(seed, length, k, repeats=6, tandem=tandem, snp_every=350)
    genome = hap[0]
    rng = cases.SplitMix(seed * 31 + k)
    raw = cases.cut_gaps(seed, genome, k, FUZ, ngaps, 10, 160, D_ERR)
    sets, gaps, gap_set = [], [], []
    for i, g in enumerate(raw):
        pos = genome.find(g["left"]) + len(g["left"])
        lo, hi = max(0, pos - 150), min(len(genome), pos + g["true_len"] + 150)
        o = rng.randint(0, len(genome) - 400)
        reads = [h[lo:hi] for h in hap] + [genome[o:o + 400]]
        reads = reads * solid
        if i % 4 == 3:
            sets[-1].extend(reads)
        else:
            sets.append(reads)
        gaps.append(g)
        gap_set.append(len(sets) - 1)
    sets.append([genome[:600]] * solid)  # named by no gap
    sets.append([])
    gaps.append(dict(raw[0]))
    gap_set.append(len(sets) - 1)  # the empty set
    return sets, gaps, gap_set


def _gap(product, g):
    return product.Gap(g["left"], g["right"], g["gap_len"], g["lmf"], g["rmf"])


def _fields(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.substats, r.phaseC_count, r.lengths)


def _sequence(g, r, unique):
    if r.count > 0 and (not unique or r.count == 1):
        return g["left"][:len(g["left"]) - r.left_fuz] + r.fill
    return g["left"] + "N" * g["gap_len"] + g["right"]


_oracle_cache = {}


def _oracle_sequence(seqs, g, k, solid, opts):
    key = (tuple(seqs), g["left"], g["right"], g["gap_len"], k, solid, tuple(sorted(opts.items())))
    if key not in _oracle_cache:
        if not seqs:
            _oracle_cache[key] = g["left"] + "N" * g["gap_len"] + g["right"]
        else:
            og = O.OracleGraph(seqs, k, solid)
            try:
                fa, _ = O.execute_single(og, g["left"], g["right"], g["gap_len"], k, solid=solid, d_err=D_ERR,
                                         max_fuz=max(g["lmf"], g["rmf"], FUZ), randseed=SEED, **opts)
            finally:
                og.free()
            _oracle_cache[key] = "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))
    return _oracle_cache[key]


def _check_oracle(sets, gaps, gap_set, res, k, solid, opts=None, unique=False):
    for i, g in enumerate(gaps):
        assert _sequence(g, res[i], unique) == _oracle_sequence(sets[gap_set[i]], g, k, solid, opts or {}), \
            "gap %d (set %d)" % (i, gap_set[i])


class _Sets:
    """one set graph and one session; fill(order, env) -> ([FillResult by position], g2s_timing)"""

    def __init__(self, product, monkeypatch, sets, gaps, gap_set, k, solid=1, graph=None, d_err=D_ERR, **opts):
        self.product, self.mp, self.gaps, self.gap_set = product, monkeypatch, gaps, gap_set
        self.u = graph if graph is not None else product.Graph.from_sets(sets, k, solid)
        self.sess = product.Session(self.u, 0, d_err=d_err, randseed=SEED, **opts)
        self.all = [_gap(product, g) for g in gaps]

    def fill(self, order=None, env=None):
        order = list(range(len(self.gaps))) if order is None else order
        with self.mp.context() as m:
            for v in ("G2S_RESIDENT", "G2S_RESIDENT_TEST_FALLBACK", "G2S_DEVICE_D2"):
                m.delenv(v, raising=False)
            for name, value in (env or {}).items():
                m.setenv(name, value)
            return self.sess.fill_sets([self.all[i] for i in order], [self.gap_set[i] for i in order], want_timing=True)

    def close(self):
        self.sess.destroy()
        self.u.free()


def _same(a, b, what=""):
    assert len(a) == len(b)
    for i in range(len(a)):
        assert _fields(a[i]) == _fields(b[i]), "%s gap %d" % (what, i)


def _resident(t, launches=1):
    assert t.resident_launches >= launches and t.resident_fallbacks == 0, (t.resident_launches, t.resident_fallbacks)


def test_a_set_list_is_finished_on_the_device(product, monkeypatch):
    """600 gaps, default environment: resident, no fallback; equal to the host path and to the oracle.  The list
    holds draw-dependent gaps and tracebacks with choices; one of those gives the same result first, last and in the
    reversed list, 500 others around it, every run resident."""
    k = 31
    sets, gaps, gap_set = _workload(k, 41, 599)
    assert len(gaps) == 600
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        res, t = w.fill()
        _resident(t)
        host, th = w.fill(env={"G2S_RESIDENT": "0"})
        assert th.resident_launches == 0
        _same(res, host)
        _check_oracle(sets, gaps, gap_set, res, k, 1)
        assert sum(r.count > 0 for r in res) > len(gaps) // 3
        # draws and choices
        assert t.draw_dependent_gaps > 0
        drawing = [i for i, r in enumerate(res) if r.draws > 1 and r.count > 1]
        assert drawing, "no gap with a traceback that has choices"
        x = drawing[0]
        others = [i for i in range(len(gaps)) if i != x][:500]
        for order in ([x] + others, others + [x], list(reversed(others + [x]))):
            r2, t2 = w.fill(order)
            _resident(t2)
            assert _fields(r2[order.index(x)]) == _fields(res[x])
            for pos, i in enumerate(order):
                assert _fields(r2[pos]) == _fields(res[i]), "gap %d at %d" % (i, pos)
    finally:
        w.close()
    # the stream is not consumed: a single-set session of the same seed, a resident set list, then fill_batch of the gap
    gr = product.Graph.from_sets([sets[gap_set[x]]], k, 1)
    sess = product.Session(gr, 0, d_err=D_ERR, randseed=SEED)
    try:
        with monkeypatch.context() as m:
            m.setenv("G2S_RESIDENT", "1")
            r1, t1 = sess.fill_sets([_gap(product, gaps[x])], [0], want_timing=True)
            _resident(t1)
            assert _fields(r1[0]) == _fields(res[x])
            rb, tb = sess.fill_batch([_gap(product, gaps[x])], want_timing=True)
            assert tb.resident_launches == 1 and tb.resident_fallbacks == 0
            assert _fields(rb[0]) == _fields(res[x])
    finally:
        sess.destroy()
        gr.free()


def test_a_list_of_several_groups(product, monkeypatch):
    """18 432 gaps (two groups): 384 distinct (gap, set) pairs named 48 times each in shuffled order"""
    k = 31
    sets, gaps, gap_set = _workload(k, 5, 383)
    rng = cases.SplitMix(99)
    order = [i for i in range(len(gaps)) for _ in range(48)]
    for i in range(len(order) - 1, 0, -1):
        j = rng.randint(0, i)
        order[i], order[j] = order[j], order[i]
    assert len(order) > 16384
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        res, t = w.fill(order)
        _resident(t, 2)
        once, _ = w.fill(env={"G2S_RESIDENT": "0"})
    finally:
        w.close()
    for pos, i in enumerate(order):
        assert _fields(res[pos]) == _fields(once[i]), "gap %d at %d" % (i, pos)


def test_around_the_switch(product, monkeypatch):
    k = 31
    sets, gaps, gap_set = _workload(k, 11 + k, 255)
    assert len(gaps) == 256
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        r256, t256 = w.fill()
        _resident(t256)
        h256, _ = w.fill(env={"G2S_RESIDENT": "0"})
        _same(r256, h256)
        short = list(range(255))
        r255, t255 = w.fill(short)
        assert t255.resident_launches == 0
        f255, tf = w.fill(short, env={"G2S_RESIDENT": "1"})
        _resident(tf)
        _same(r255, f255)
        _same(r255, h256[:255])
        one, t1 = w.fill([3], env={"G2S_RESIDENT": "1"})
        _resident(t1)
        assert _fields(one[0]) == _fields(h256[3])
    finally:
        w.close()


@pytest.mark.parametrize("k", [63, 95])
def test_wide_kmers(product, monkeypatch, k):
    sets, gaps, gap_set = _workload(k, 11 + k, 255)
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        res, t = w.fill()
        _resident(t)
        host, th = w.fill(env={"G2S_RESIDENT": "0"})
        assert th.resident_launches == 0
        _same(res, host)
        _check_oracle(sets, gaps, gap_set, res, k, 1)
        assert sum(r.count > 0 for r in res) > len(gaps) // 3
    finally:
        w.close()


@pytest.mark.parametrize("opt", ["all_upper", "best_only", "unique"])
def test_options(product, monkeypatch, opt):
    opts = {"all_upper": dict(skip_confident=True), "best_only": dict(all_paths=False), "unique": dict(unique_paths=True)}[opt]
    k = 31
    sets, gaps, gap_set = _workload(k, 23, 299, solid=2)
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k, solid=2, **opts)
    try:
        res, t = w.fill()
        _resident(t)
        host, th = w.fill(env={"G2S_RESIDENT": "0"})
        assert th.resident_launches == 0
        _same(res, host)
        _check_oracle(sets, gaps, gap_set, res, k, 2, opts, unique=opt == "unique")
    finally:
        w.close()


# (k, seed) of a toy workload whose closures the fill kernels leave to phase D2: tandem arrays at a short k put a k-mer
# at several depths of a closure.  Found by trying seeds on the device (the first of range(40, 60) at k = 21 with a
# non-zero count).
HOST_FINISHED = (21, 40)


def test_gaps_the_host_finishes(product, monkeypatch):
    """G2S_DEVICE_D2=0: the closures the fill kernels do not analyse go to the host's threads from the hand-off, with
    their rand() values from value 0; the same list with phase D2 on the device"""
    k, seed = HOST_FINISHED
    sets, gaps, gap_set = _workload(k, seed, 399, tandem=40, length=6000)
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        res, t = w.fill(env={"G2S_DEVICE_D2": "0"})
        _resident(t)
        print("host_finished_gaps", t.host_finished_gaps)
        assert t.host_finished_gaps > 0
        host, th = w.fill(env={"G2S_RESIDENT": "0"})
        assert th.resident_launches == 0
        _same(res, host)
        dev, td = w.fill(env={"G2S_DEVICE_D2": "1"})
        _resident(td)
        _same(dev, host)
    finally:
        w.close()


def test_a_list_the_device_gives_back(product, monkeypatch):
    k = 31
    sets, gaps, gap_set = _workload(k, 59, 299)
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        base, t = w.fill()
        _resident(t)
        res, tf = w.fill(env={"G2S_RESIDENT_TEST_FALLBACK": "1"})
        assert tf.resident_fallbacks >= 1 and tf.resident_launches == 0
        _same(res, base)
        again, ta = w.fill()  # (and the session takes the next list on the device again)
        _resident(ta)
        _same(again, base)
    finally:
        w.close()


def test_kernel_paths_change_nothing(product, monkeypatch):
    k = 31
    sets, gaps, gap_set = _workload(k, 59, 299)
    w = _Sets(product, monkeypatch, sets, gaps, gap_set, k)
    try:
        base, t = w.fill()
        _resident(t)
        assert t.traced_in_fill_gaps > 0
        for env in (("G2S_SEG_WAVES", "1"), ("G2S_SEG_WAVES", "2"), ("G2S_TRACE_WAVES", "1"), ("G2S_TRACE_WAVES", "4"),
                    ("G2S_TRACE_IN_FILL", "0"), ("G2S_TRACE_GUESS", "0"), ("G2S_TRACE_GUESS", "1")):
            res, te = w.fill(env=dict([env]))
            _resident(te)
            _same(res, base, "%s=%s:" % env)
            if env == ("G2S_TRACE_IN_FILL", "0"):
                assert te.traced_in_fill_gaps == 0
    finally:
        w.close()


def test_a_pooled_graph(product, monkeypatch):
    k = 31
    seqs, set_lists, shared, set_shared, gaps, gap_set = PC.fill_workload(k, 42, 270)
    assert len(gaps) >= 256
    u = product.Graph.from_pool(seqs, set_lists, k, 1, shared=shared, set_shared=set_shared)
    w = _Sets(product, monkeypatch, None, gaps, gap_set, k, graph=u, d_err=PC.D_ERR)
    try:
        res, t = w.fill()
        _resident(t)
        host, th = w.fill(env={"G2S_RESIDENT": "0"})
        assert th.resident_launches == 0
        _same(res, host)
        assert sum(r.count > 0 for r in res) > len(gaps) // 3
    finally:
        w.close()


def _set_race_hunt(runs, library):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "gap2seq_amd", library, "libg2s_hip.so") if library else os.path.join(root, "gap2seq_amd", "libg2s_hip.so")
    if not os.path.exists(so):
        pytest.fail("%s is missing: __graft_entry__.build() makes it" % so)
    env = dict(os.environ, G2S_LIBRARY=so)
    for v in ("G2S_RESIDENT", "G2S_DEVICE_D2", "G2S_FORCE_SEGX", "G2S_NO_SEG_TIER", "G2S_RESIDENT_TEST_FALLBACK"):
        env.pop(v, None)
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "race_hunt_sets.py"), str(runs)], env=env, capture_output=True,
                         text=True, timeout=600)
    rows = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert rows, "race_hunt_sets.py with %s (exit %d): %s" % (library or "the product build", out.returncode, out.stderr[-2000:])
    return rows[-1]


def test_race_hunting_builds_give_the_product_builds_results_on_a_set_list():
    """tools/race_hunt_sets.py: a resident set list of 600 gaps 20 times with the product build, the jitter build and
    the paranoid build (csrc/sync_debug.h): no call differs from its build's first, the three builds agree"""
    rows = [_set_race_hunt(20, lib) for lib in ("", "_jit", "_par")]
    for r in rows:
        assert r["differ"] == 0, "%s: %d of %d calls differ from the first" % (r["library"], r["differ"], r["runs"])
        assert r["resident_launches"] >= 1 and r["fallbacks"] == 0 and r["filled"] > r["gaps"] // 3, r
    assert len({r["digest"] for r in rows}) == 1, "the builds disagree: %r" % [(r["library"], r["digest"]) for r in rows]
