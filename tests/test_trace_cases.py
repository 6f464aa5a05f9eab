"""The designed tracebacks of tests/trace_cases.py on the CPU, before tests/test_gpu_trace_designed.py takes them to the
device: a row that is not what its table entry says fails here, where it is written.

Every row through the segment tier's model (closure segments, hops, path lengths, stop depths, the route predicate of
tests/trace_model.py at every -dist-error of its list), through test_seg_model's chain (model = oracle state by state,
the host's phase D of post.cpp on the model's closure = oracle in count, fuz, draws, fill text and case, statistics)
and against the string restatement oracle/pyref.py; the oracle's own text has the lower-case bases where the design
puts them; both path lengths and both stop depths occur over the copies of a list.  The ladders the suite had before
(cases.EDGE_LADDERS, cases.LIMIT_EDGES) come out of the extended generator as they did: tests/golden/ladder_digests.json.

The whole file takes about 10 s on one core (the digests of the 16 384-segment ladders 4 s of them)."""
import hashlib
import json
import os
import re

import pytest

import cases
import pyref
import trace_cases as TC
import trace_model as TM
from test_seg_model import check_config

K = TC.K
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = list(TC.ROWS)
_LIST_ORACLE = {}


def _digest(lad):
    return hashlib.sha256(json.dumps([lad["seqs"], lad["gap"]], sort_keys=True).encode()).hexdigest()[:16]


def test_the_old_ladders_are_byte_identical():
    """bubble_ladder's new arguments (run, run_step, del_len) leave every ladder of the old tables as it was: the
    digests were taken from the generator before it was extended."""
    want = json.load(open(os.path.join(HERE, "golden", "ladder_digests.json")))
    assert sorted(want) == sorted(list(cases.EDGE_LADDERS) + list(cases.LIMIT_EDGES))
    got = {n: _digest(cases.edge_ladder(n)[0]) for n in cases.EDGE_LADDERS}
    got.update({n: _digest(cases.limit_edge(n)[0]) for n in cases.LIMIT_EDGES})
    assert got == want


def test_the_new_arguments_do_what_they_say():
    a = cases.bubble_ladder(7, K, 1, 32 + 60, lead=10, tail=10, run=60, run_step=20)
    g, h = a["seqs"]
    assert len(g) == len(h) and [i for i in range(len(g)) if g[i] != h[i]] == [K + 3 + 10 + q for q in (0, 20, 40, 60)]
    b = cases.bubble_ladder(7, K, 1, 32, lead=10, tail=10, indel=True, indel_every=1, del_len=2)
    g, h = b["seqs"]
    assert len(h) == len(g) - 2 and h == g[:K + 3 + 10] + g[K + 3 + 12:]
    assert b["gap"]["true_len"] == 10 + 1 + 10 + 1


def _list_of(name):
    return TC.ROWS[name]["list"]


def _routes(product, lst, e):
    seqs, gaps, idx = TC.trace_list(lst)
    L = TC.LISTS[lst]
    return TC.list_routes(product, seqs, gaps, e, L["skip"], bool(L["env"].get("G2S_DEVICE_D2")), key=(lst, e))


@pytest.mark.parametrize("name", NAMES)
def test_row_is_what_its_table_entry_says(product, name):
    """ncl, hops, len, stops, sure and — with the dmax of the row's LIST — the route at every -dist-error of the list."""
    lst = _list_of(name)
    want = TC.ROWS[name]["want"]
    seqs, gaps, idx = TC.trace_list(lst)
    assert len(idx[name]) == TC.ROWS[name]["copies"]
    for e in TC.LISTS[lst]["d_errs"]:
        routes, dmax = _routes(product, lst, e)
        r = routes[idx[name][0]]
        assert r is not None, name
        assert (r["ncl"], r["hops"], r["fill"]["len0"], r["fill"]["sure"]) == (want["ncl"], want["hops"], want["len"][0], want["sure"]), (name, e, r)
        if "stops" in want:
            assert r["stops"] == want["stops"], (name, r["stops"])
        if "way" in want:
            assert r["way"] == want["way"][e], (name, e, r["way"], r["L"] * r["nsegs"], 2 * r["map_cap"])
        if "takes" in want:
            assert r["fill"]["takes"] == want["takes"], (name, r["fill"])
        if r["way"] != "big" and not TC.LISTS[lst]["skip"]:
            assert r["nseg"] <= TM.FILL_ANALYSED_SEGS, (name, r["nseg"])  # the fill kernel analyses the closure itself
        # the regular tier keeps the gap (256 right-set entries, 512 logged segments, 64 pending events): at the list's
        # first -dist-error every row; a larger one widens the right set over more in-tips, two entries each
        assert r["fill"]["regular"] == (r["nA"] <= 256), (name, e, r["nA"])
        if e == TC.LISTS[lst]["d_errs"][0]:
            assert r["fill"]["regular"], (name, e, r["nA"], r["nseg"])
        # the planted gaps set the list's dmax: every pad lies below every planted gap
        planted = {i for v in idx.values() for i in v}
        assert max(TM.gap_d(g, e) for i, g in enumerate(gaps) if i not in planted) < min(TM.gap_d(gaps[i], e) for i in planted)


def test_every_route_is_taken_below_on_and_above_64_and_128_hops(product):
    """The table as a whole: jump, unguessed chase (rows the fill wave takes outright, with G2S_TRACE_IN_FILL=0) and
    guessed chase (rows with a choice) at 63 to 65 and 127 to 129 hops; one and two segments (L = 0 and 1: 0 and 2 are
    below 2 * map_cap whatever the list, so these can only jump); the walk through device memory at 63 to 65 and 128."""
    took = {}
    for name, r in TC.ROWS.items():
        w = r["want"]
        for e, way in w.get("way", {}).items():
            took.setdefault((way, w["sure"]), set()).add(w["hops"][0][0])
    both = {63, 64, 65, 127, 128, 129}
    assert both <= took[("jump", True)] and both <= took[("chase", True)]
    assert both <= took[("jump", False)] and both <= took[("chase", False)]
    assert {1, 2} <= took[("jump", True)]
    assert {63, 64, 65, 128} <= took[("big", False)] and max(took[("big", True)]) > 256
    # the bound itself: L * ncl == 2 * map_cap
    r64, _ = _routes(product, "chain64", 14)
    r128, _ = _routes(product, "chain128", 237)
    i64, i128 = TC.trace_list("chain64")[2]["p64"][0], TC.trace_list("chain128")[2]["p128"][0]
    assert (r64[i64]["L"] * 64, r64[i64]["map_cap"], r64[i64]["jump"]) == (384, 192, True)
    assert (r128[i128]["L"] * 128, r128[i128]["map_cap"], r128[i128]["jump"]) == (896, 448, True)
    # and one step of map_cap below it the same gaps chase
    assert _routes(product, "chain64", 10)[0][i64]["map_cap"] == 188 and _routes(product, "chain128", 233)[0][i128]["map_cap"] == 444


@pytest.mark.parametrize("name", NAMES)
def test_row_through_the_model_the_hosts_phase_d_and_the_oracle(product, oracle, name):
    """test_seg_model's chain on the row alone on its graph: states, counters, closure, and post.cpp's analysis and
    traceback on that closure are the oracle's, field by field; no Q7."""
    r = TC.row(name)
    L = TC.LISTS[_list_of(name)]
    for e in L["d_errs"][:2]:
        assert check_config(product, oracle, r["seqs"], K, [r["gap"]], e, skip=L["skip"]) == (1, 0)


@pytest.mark.parametrize("name", [n for n in NAMES if TC.ROWS[n]["list"] in ("chain64", "case", "lens")])
def test_row_equals_the_python_restatement(oracle, name):
    r = TC.row(name)
    g = r["gap"]
    og = oracle.OracleGraph(r["seqs"], K, 1)
    rng = oracle.OracleRng(5)
    try:
        o = oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], 10, g["lmf"], g["rmf"])
    finally:
        rng.free()
        og.free()
    pi = pyref.Info()
    c2, lf2, rf2, fill2, sub2 = pyref.fill_gap(pyref.Graph(r["seqs"], K, 1), pyref.GlibcRand(5), g["left"], g["right"],
                                               g["gap_len"], 10, g["lmf"], g["rmf"], False, True, True, pi)
    assert (o.count, o.left_fuz, o.right_fuz) == (c2, lf2, rf2)
    assert (o.info.phaseC_count, o.lengths, o.info.draws, o.info.q7) == (pi.phaseC_count, pi.lengths, pi.draws, pi.q7)
    assert o.fill == pyref.fill_string(fill2, g["lmf"] - lf2)


def _oracle_list(oracle, lst):
    """The oracle's results for a whole list at its first -dist-error, one rand() stream from seed 5 on, as the device
    legs run it (computed once)."""
    if lst not in _LIST_ORACLE:
        seqs, gaps, idx = TC.trace_list(lst)
        L = TC.LISTS[lst]
        og = oracle.OracleGraph(seqs, K, 1)
        rng = oracle.OracleRng(5)
        try:
            _LIST_ORACLE[lst] = [oracle.fill_gap(og, rng, g["left"], g["right"], g["gap_len"], L["d_errs"][0], g["lmf"], g["rmf"], L["skip"], True)
                                 for g in gaps]
        finally:
            rng.free()
            og.free()
    return _LIST_ORACLE[lst]


@pytest.mark.parametrize("lst", list(TC.LISTS))
def test_list_is_clean_padded_and_within_the_segment_buffer(product, oracle, lst):
    """One graph without a repeated or strand-meeting k-mer, at least 256 gaps, no Q7 case (every gap is compared), the
    copies' results those of the row alone, under 64 closure segments a gap on average."""
    seqs, gaps, idx = TC.trace_list(lst)
    assert cases.clean_haplotypes(seqs, K) and len(gaps) >= 256
    res = _oracle_list(oracle, lst)
    assert not any(o.info.q7 for o in res)
    routes, _ = _routes(product, lst, TC.LISTS[lst]["d_errs"][0])
    assert sum(r["ncl"] for r in routes if r) < 64 * len(gaps)
    for name, at in idx.items():
        want = TC.ROWS[name]["want"]
        for i in at:
            assert res[i].phase_d and res[i].count > 0 and res[i].lengths == want["len"], (name, i)


@pytest.mark.parametrize("name", [n for n in NAMES if "low" in TC.ROWS[n]["want"]])
def test_case_rows_have_their_lower_case_where_the_design_puts_it(oracle, name):
    """The oracle's text of every copy (each at another place of the rand() stream: both arms are taken): the unsafe
    run is the k-mers that hold a substitution, J' + k of them; its lower-case bases are the J' + 1 that lie k or more
    below the safe base above, the first exactly k below it.  In threads of the four-wave kernel (one base a thread up
    to 256 bases, from the top of the fill) the safe base and the run's lowest state sit where the row says."""
    row, want, gen = TC.row(name), TC.ROWS[name]["want"], TC.ROWS[name]["gen"]
    seqs, gaps, idx = TC.trace_list("case")
    res = _oracle_list(oracle, "case")
    step = gen.get("run_step") or K - 1
    jp = gen.get("run", 0) // step * step
    a, b = gen["lead"], gen["lead"] + jp
    assert want["low"] == (a, b)
    texts = set()
    for i in idx[name]:
        f = res[i].fill
        texts.add(f)
        assert len(f) == want["len"][0] - 3 and res[i].left_fuz == 0
        assert [(m.start(), m.end() - 1) for m in re.finditer("[acgt]+", f)] == [(a, b)], (name, i)
        top = len(f) - 1
        if "safe" in want:
            assert len(f) <= 256 and (top - (b + K), top - a) == (want["safe"], want["bottom"])
    assert len(texts) == 2  # both arms over the copies
    if name == "r61same":
        assert want["safe"] >> 6 == want["bottom"] >> 6 == 1
    elif name in ("r61cross", "r64", "r65"):
        assert want["bottom"] - want["safe"] == dict(r61cross=61, r64=64, r65=65)[name] and (want["safe"] >> 6, want["bottom"] >> 6) == (0, 1)
    elif name == "r121":
        assert (want["safe"] >> 6, want["bottom"] >> 6) == (0, 2)  # the word of the wave two in front
    elif name == "r181":
        assert (want["safe"] >> 6, want["bottom"] >> 6) == (0, 3) and want["bottom"] - want["safe"] > 128  # wave 3 reads all three words
    elif name == "r331":
        assert (want["len"][0] - 3 + 255) // 256 == want["per"] == 2
    elif name == "snp35":  # one lane of a one-wave kernel holds the safe base below the run, the run and the safe base above it
        n = want["len"][0] - 3
        per = (n + 63) // 64
        assert per == want["per1"] and (n - 1 - (a - 1)) // per == (n - 1 - (b + K)) // per


def test_both_lengths_and_both_stops_occur_over_the_copies(oracle):
    for lst, sfx in (("lens", ""), ("lens-skip", "/skip")):
        seqs, gaps, idx = TC.trace_list(lst)
        res = _oracle_list(oracle, lst)
        # (the fill begins at depth stop + 1 = lmf - left_fuz + 1 and ends at the path's length)
        lens = lambda name: {len(res[i].fill) + 3 - res[i].left_fuz for i in idx[name + sfx]}
        fuz = lambda name: {res[i].left_fuz for i in idx[name + sfx]}
        assert lens("two-lengths") == {101, 99} and fuz("two-lengths") == {0}
        assert lens("two-stops") == {93} and fuz("two-stops") == {0, 2}
        assert lens("two-lengths-two-stops") == {79, 77} and fuz("two-lengths-two-stops") == {0, 2}
        # the first length is the longer in every row: phase C lists base + err in front of base - err (:1125-1126), so
        # a guess — the first length — is the longer path, and a gap whose rand() picks the second is the shorter
        for name in idx:
            w = TC.ROWS[name]["want"]["len"]
            assert w == sorted(w, reverse=True)


def test_two_lengths_are_guessed_only_under_the_skip_rule(product):
    """A closure with two path lengths holds its reached k-mer at two depths: the fill kernel leaves it to phase D2
    and its wave does not guess; under the skip rule nothing is analysed and the wave guesses the longer length."""
    for lst, takes in (("lens", False), ("lens-skip", True)):
        idx = TC.trace_list(lst)[2]
        routes, _ = _routes(product, lst, 10)
        for name, at in idx.items():
            f = routes[at[0]]["fill"]
            two = len(TC.ROWS[name]["want"]["len"]) == 2
            assert f["takes"] == (takes or not two) and not f["sure"], (name, f)
            if lst == "lens":  # (under the skip rule no state is looked at as being on a path to a sink)
                assert f["dag"] == (not two), (name, f)


def test_the_fill_waves_counts_by_the_model(product):
    """What tests/test_gpu_trace_designed.py asserts traced_in_fill_gaps and guessed_in_fill_gaps against: the planted
    copies the design says, and the pads (plain gaps: one path each)."""
    for lst, e, planted_traced, planted_guessed in (("chain64", 10, 10, 48), ("chain128", 10, 6, 48), ("case", 10, 0, 128),
                                                    ("lens", 10, 0, 16), ("lens-skip", 10, 0, 48), ("fillcap", 10, 8, 0), ("deep", 10, 4, 0),
                                                    # (128 in-tips inside the right set are 257 entries and more: the large variant's)
                                                    ("chain128", 233, 2, 16)):
        seqs, gaps, idx = TC.trace_list(lst)
        routes, _ = _routes(product, lst, e)
        planted = [i for v in idx.values() for i in v]
        t, g = TC.fill_counts([routes[i] for i in planted], True)
        assert (t, g) == (planted_traced, planted_guessed), lst
        pads = [r for i, r in enumerate(routes) if i not in set(planted)]
        assert all(r is None or (r["fill"]["sure"] and r["fill"]["takes"]) for r in pads)
