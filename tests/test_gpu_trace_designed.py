"""The designed tracebacks of tests/trace_cases.py on the device (run with `-m gpu` on an MI355X): the chain of segments
by pointer jumping, by both hop-by-hop chases and through device memory at 63 / 64 / 65 and 127 / 128 / 129 hops, on
either side of L * nsegs <= 2 * map_cap and on it; the case rule across a lane, a wave and two waves and with several
bases a thread; two path lengths and two stop depths, each taken by some copy; the fill wave's own tracer at 255 / 256 /
257 closure records and at path lengths 4095 / 4096 / 4097.  tests/test_trace_cases.py proves on the CPU that every row
is what the table says and that the model (tests/trace_model.py) routes it as designed.

Every list runs on every leg — one and four waves a gap in the trace kernel, guesses off, every gap guessing, the fill
wave's tracer off, the trace kernel behind g2s_d3_back, the host path — and every leg is compared with the oracle field
by field (count, fuz, draws, fill text AND case, statistics), every leg with every other, and finished on the device
without a fallback: a bad verdict of a walk would send the list to the host path, whose equal results would hide the
kernel.  traced_in_fill_gaps and guessed_in_fill_gaps are the model's counts.  guessed_groups and
guessed_groups_resent are added after a wave has been counted as finished and can land in the next list: only
resent <= groups is asserted.

On an MI355X the whole file takes 10 s."""
import pytest

import trace_cases as TC
from d2_witness import _run_logged
from test_gpu_edges import _seg_dump
from test_gpu_parity import _compare_with_oracle_in_parallel, _gaps

pytestmark = pytest.mark.gpu
K = TC.K
SEED = 5
SWITCHES = ("G2S_TRACE_WAVES", "G2S_TRACE_GUESS", "G2S_GUESS_PERCENT", "G2S_TRACE_IN_FILL", "G2S_D3_BACK", "G2S_DEVICE_D2",
            "G2S_RESIDENT", "G2S_D2_BIG", "G2S_NO_EARLY_SEGW", "G2S_SEG_WAVES", "G2S_NO_SEG_TIER", "G2S_FORCE_SEGX",
            "G2S_NO_SEGX_TIER")
_RES = dict(G2S_RESIDENT="1")
# guess: None — which gaps guess depends on the waves' timing (the first 87 % of a short list in the order their searches
# end) —, True — every gap that can —, False — none
LEGS = {
    "four-waves": (dict(_RES, G2S_TRACE_WAVES="4"), None),
    "one-wave": (dict(_RES, G2S_TRACE_WAVES="1"), None),
    "no-guess": (dict(_RES, G2S_TRACE_GUESS="0"), False),
    "no-guess-one-wave": (dict(_RES, G2S_TRACE_GUESS="0", G2S_TRACE_WAVES="1"), False),
    "all-guess": (dict(_RES, G2S_GUESS_PERCENT="100"), True),
    "all-guess-one-wave": (dict(_RES, G2S_GUESS_PERCENT="100", G2S_TRACE_WAVES="1"), True),
    "not-in-fill": (dict(_RES, G2S_TRACE_IN_FILL="0"), False),
    "not-in-fill-one-wave": (dict(_RES, G2S_TRACE_IN_FILL="0", G2S_TRACE_WAVES="1"), False),
    "in-fill": (dict(_RES, G2S_TRACE_IN_FILL="1"), None),
    "back": (dict(_RES, G2S_D3_BACK="1"), None),
    "back-not-in-fill": (dict(_RES, G2S_D3_BACK="1", G2S_TRACE_IN_FILL="0"), False),
    "host-path": (dict(G2S_RESIDENT="0"), None),
}


@pytest.fixture(scope="module")
def graphs(product, oracle):
    """{list: (product graph, oracle graph)}, built when a list is first asked for, freed with the module."""
    made = {}

    def get(lst, seqs):
        if lst not in made:
            made[lst] = (product.Graph.from_seqs(seqs, K, 1), oracle.OracleGraph(seqs, K, 1))
        return made[lst]

    yield get
    for pg, og in made.values():
        pg.free()
        og.free()


def _key(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, tuple(r.substats), r.phaseC_count, tuple(r.lengths))


def _leg(product, oracle, monkeypatch, pg, og, gaps, e, skip, env):
    """One call of the list under `env`: (results as keys, timing), compared with the oracle gap by gap."""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for kv in env.items():
        monkeypatch.setenv(*kv)
    sess = product.Session(pg, 0, d_err=e, skip_confident=skip, randseed=SEED)
    try:
        before = product.test_d3_chain_launches()
        res, tm = sess.fill_batch(_gaps(product, gaps), True)
        tm.chain_taken = product.test_d3_chain_launches() - before  # (the route with the chain walked by g2s_d3_trace<4, true>)
    finally:
        sess.destroy()
        for v in env:
            monkeypatch.delenv(v, raising=False)
    assert tm.watchdog_gaps == 0
    compared, q7 = _compare_with_oracle_in_parallel(product, oracle, og, gaps, res, e, SEED, skip=skip, threads=16)
    assert (compared, q7) == (len(gaps), 0)  # (the designs hold no Q7 case and no memory verdict: every gap is compared)
    return [_key(r) for r in res], tm


def _all_legs(product, oracle, monkeypatch, graphs, lst, e, legs, seqs_gaps=None):
    seqs, gaps, idx = seqs_gaps or TC.trace_list(lst)
    L = TC.LISTS[lst]
    pg, og = graphs(lst if seqs_gaps is None else lst + "+long", seqs)
    by_runs = bool(L["env"].get("G2S_DEVICE_D2"))
    routes, dmax = TC.list_routes(product, seqs, gaps, e, L["skip"], by_runs, key=(lst, e, len(gaps)))
    first = None
    for leg in legs:
        env, guess = LEGS[leg]
        env = dict(env, **(L["env"] if env.get("G2S_RESIDENT") == "1" else {}))
        keys, tm = _leg(product, oracle, monkeypatch, pg, og, gaps, e, L["skip"], env)
        if first is None:
            first = keys
        assert keys == first, "%s at -dist-error %d: leg %s differs from leg %s" % (lst, e, leg, legs[0])
        if env.get("G2S_RESIDENT") != "1":
            continue
        assert tm.resident_launches == 1 and tm.resident_fallbacks == 0, (lst, e, leg)
        # which trace kernel ran, by the library's own count (d3_device.hip, launch_d3): up to 768 gaps on four waves
        # g2s_d3_trace<4, true>, which walks the chain of draws itself; behind g2s_d3_back, on one wave a gap, and on a list
        # of more than 768 gaps — the one-wave kernel behind g2s_d3_blocks / g2s_d3_chain / g2s_d3_handoff — the plain one
        short = len(gaps) <= 768 and "G2S_D3_BACK" not in env and env.get("G2S_TRACE_WAVES") != "1"
        if lst in ("chain64", "chain128"):
            assert tm.chain_taken == (1 if short else 0), (lst, e, leg, tm.chain_taken)
        in_fill = env.get("G2S_TRACE_IN_FILL") != "0"
        traced, guessed = TC.fill_counts(routes, True)
        print("%s d_err %d %-22s chain %d traced %d (model %d) guessed %d (model %d) groups %d resent %d" % (
            lst, e, leg, tm.chain_taken, tm.traced_in_fill_gaps, traced if in_fill else 0, tm.guessed_in_fill_gaps, guessed, tm.guessed_groups,
            tm.guessed_groups_resent))
        assert tm.traced_in_fill_gaps == (traced if in_fill else 0), (lst, e, leg)
        if not in_fill or guess is False:
            assert tm.guessed_in_fill_gaps == 0, (lst, e, leg)
        elif guess:
            assert tm.guessed_in_fill_gaps == guessed, (lst, e, leg)
        else:
            assert tm.guessed_in_fill_gaps <= guessed, (lst, e, leg)
        assert tm.guessed_groups_resent <= tm.guessed_groups
    return routes


CHAIN = [(lst, e) for lst in ("chain64", "chain128") for e in TC.LISTS[lst]["d_errs"]]


@pytest.mark.parametrize("lst,e", CHAIN)
def test_chain_routes(product, oracle, monkeypatch, graphs, lst, e):
    """The chain at 1, 2, 63 to 65 and 127 to 129 hops.  At this list's map_cap the model says which rows jump and which
    chase (tests/trace_cases.py: `way`); a row the fill wave takes outright reaches the trace kernel's unguessed chase
    with G2S_TRACE_IN_FILL=0, a row with a choice with G2S_TRACE_GUESS=0, and the guessed chase with every gap
    guessing; each on four waves a gap and on one, and behind g2s_d3_back (the kernel without the chain's walk)."""
    routes = _all_legs(product, oracle, monkeypatch, graphs, lst, e, list(LEGS))
    idx = TC.trace_list(lst)[2]
    assert {n: routes[idx[n][0]]["way"] for n in idx} == {n: TC.ROWS[n]["want"]["way"][e] for n in idx}


@pytest.mark.parametrize("lst", ["case", "lens", "lens-skip"])
def test_case_rule_and_path_lengths(product, oracle, monkeypatch, graphs, lst):
    """Unsafe runs of 61, 64, 65, 121 and 331 states (the nearest safe base in the same wave, in the wave in front,
    two waves in front; two bases a thread) and an SNP's run inside one lane's stretch of a one-wave kernel; gaps with
    two path lengths and with two stop depths, every copy at another place of the rand() stream: a guess is the first
    length and the first parent, the copies that draw the other length or arm are sent again by the trace kernel (two
    lengths are guessed only under the skip rule: the list "lens-skip")."""
    _all_legs(product, oracle, monkeypatch, graphs, lst, 10, list(LEGS))


def test_fill_waves_record_bound(product, oracle, monkeypatch, graphs):
    """255 and 256 closure records and hops are the fill wave's (nrec <= 256; nh >= 256 gives up BEFORE hop 257 only),
    257 the trace kernel's; under the skip rule, where a closure of that size is still the fill kernel's own."""
    routes = _all_legs(product, oracle, monkeypatch, graphs, "fillcap", 10,
                       ["in-fill", "one-wave", "not-in-fill", "not-in-fill-one-wave", "back", "host-path"])
    idx = TC.trace_list("fillcap")[2]
    assert [routes[idx[n][0]]["fill"]["takes"] for n in ("rec255", "rec256", "rec257")] == [True, True, False]


def test_fill_waves_length_bound(product, oracle, monkeypatch, graphs):
    """Path lengths 4095 and 4096 are the fill wave's (len0 <= 4096: its text buffer), 4097 the trace kernel's; the
    list is deep, and G2S_NO_EARLY_SEGW=1 keeps its longest gaps in the regular tier."""
    routes = _all_legs(product, oracle, monkeypatch, graphs, "deep", 10, ["in-fill", "one-wave", "not-in-fill", "host-path"])
    idx = TC.trace_list("deep")[2]
    assert [routes[idx[n][0]]["fill"]["takes"] for n in ("len4095", "len4096", "len4097")] == [True, True, False]


@pytest.mark.parametrize("e", TC.LISTS["big"]["d_errs"])
def test_walk_through_device_memory(product, oracle, monkeypatch, graphs, e):
    """Closures of more than 192 segments, analysed by g2s_d2_*, at 63, 64, 65 and 128 hops, and one of 401: its runs in
    device memory at -dist-error 10 (2 * n_runs > map_cap = 752) and in LDS at 100 (map_cap 840).  The device's n_runs
    is not read — the DAG route leaves it out of G2S_D2_LOG, and the host's hook does not return it —: the assertion
    below is arithmetic on the model's segments with the margin of d2_device.hip's rule (a run a segment, two where a
    sink splits one: 401 to 403), and the two sides of `2 * n_runs <= map_cap` are shown by equal results alone."""
    routes = _all_legs(product, oracle, monkeypatch, graphs, "big", e, ["four-waves", "one-wave", "no-guess", "back", "host-path"])
    idx = TC.trace_list("big")[2]
    assert all(routes[idx[n][0]]["way"] == "big" for n in idx)
    r = routes[idx["runs401"][0]]
    # (a run a segment, two where a sink splits one: d2_device.hip — 401 to 403 runs)
    assert (2 * (r["ncl"] + 2) <= r["map_cap"]) == (e == 100) and (2 * r["ncl"] > r["map_cap"]) == (e == 10)


def test_long_list_with_the_chain_rows(product, oracle, monkeypatch, graphs):
    """More than 768 gaps: the one-wave trace kernel behind g2s_d3_handoff, with the rows of both chain lists; that no
    leg took the short list's kernel is the library's own count (g2s_test_d3_chain_launches, in _all_legs)."""
    seqs, gaps, idx = TC.long_chain_list()
    assert len(gaps) > 768
    routes = _all_legs(product, oracle, monkeypatch, graphs, "chain64", 10, ["in-fill", "not-in-fill", "no-guess", "all-guess"],
                       seqs_gaps=(seqs, gaps, idx))
    ways = {routes[idx[n][0]]["way"] for n in idx}
    assert ways == {"jump", "chase"}


@pytest.mark.parametrize("lst", ["chain64", "chain128", "fillcap", "case", "lens", "lens-skip", "deep"])
def test_the_kernels_count_the_models_segments(product, monkeypatch, tmp_path, lst):
    """The fill kernel's own dump: every planted gap logged the segments the model says (on the chain rows one more
    than the closure has: the left seeds' stretch) — the route predicate stands on the device's number."""
    seqs, gaps, idx = TC.trace_list(lst)
    routes, _ = TC.list_routes(product, seqs, gaps, 10, TC.LISTS[lst]["skip"], False, key=(lst, 10, len(gaps)))
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    recs, tm, res = _seg_dump(product, monkeypatch, tmp_path, seqs, gaps, "2")
    for n, at in idx.items():
        for i in at:
            assert [x[1] for x in recs[i]] == [routes[i]["nseg"]], (n, i, recs[i])
            if lst in ("chain64", "chain128", "fillcap"):
                assert routes[i]["nseg"] == routes[i]["ncl"] + 1, (n, routes[i]["nseg"], routes[i]["ncl"])


def test_d2_takes_the_big_rows_with_the_models_closure(product, tmp_path):
    """The library's own log of phase D2 (a child process: the switch is read once): every row of the `big` list was
    taken by a g2s_d2_* kernel with the model's closure segments."""
    seqs, gaps, idx = TC.trace_list("big")
    names = list(idx)
    by, r = _run_logged(tmp_path, dict(trace="big", d_err=10), names, 300, dict(G2S_D2_BIG="1"))
    routes, _ = TC.list_routes(product, seqs, gaps, 10, False, True, key=("big", 10, len(gaps)))
    for n in names:
        rows = by[n]
        print(n, rows, routes[idx[n][0]]["ncl"], routes[idx[n][0]]["ncl_s"])
        r = routes[idx[n][0]]
        # (nrec: the closure's records; ns: its segments on a path to a sink, counted where the closure is no DAG)
        assert rows and rows[-1]["rc"] == 0 and rows[-1]["nrec"] == r["ncl"] and rows[-1]["ns"] in (0, r["ncl_s"]), (n, rows)
        assert (rows[-1]["ns"] == 0) == r["fill"]["dag"], (n, rows)
        assert rows[-1]["kernel"] == (1 if TC.ROWS[n]["want"]["ncl"] > 256 else 0), (n, rows)
