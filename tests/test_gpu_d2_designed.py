"""Phase D2 on designed cyclic closures, on every path it can take (run with `-m gpu` on an MI355X).

tests/d2_cases.py holds fifteen gaps whose closure has a known strong-component structure — tandem arrays (a cycle),
a 2-cycle, a self loop, components in series and on parallel arms, a chord, a figure of eight, a loop inside a
component, cycles that hold the sink positions or the seeds, a cycle in front of a bubble ladder — and
tests/test_d2_cases.py proves on the CPU that each has it.  Here the designs of one -dist-error form one list on one
graph among 100 ordinary gaps (four lists: the comparison takes -dist-error per list), every field of every result is
compared with the oracle (test_gpu_parity._check_batch: count, fuz, draws, fill text and case, the six subgraph
statistics), on the device's default path, on each of its test switches, on the host's threads and on the host path.

The witnesses (one child process per list, as the log's switch is read once per process) keep a design from passing
by a detour: the library's own log (G2S_D2_LOG) must show which g2s_d2_* kernel took which design.  g2s_d2_small holds
256 closure segments; the model (d2_cases: ncl) says which designs are beyond that: two-cycle, self-loop, series-3,
loop-in-component and both cycle+bubbles.  On a list that is not deep the library launches no large instantiation by
default (g2s_api.hip: d2_big), and what the small one passes on is the host's: test_small_instantiation_alone pins
that; test_every_design_is_taken_by_a_d2_kernel runs with G2S_D2_BIG=1, the large instantiation behind the small
one on every list, and there every design must be taken on the device."""
import pytest

import d2_cases as DC
from d2_witness import d2_log_of_designs
from test_gpu_parity import _check_batch

pytestmark = pytest.mark.gpu
K = DC.K
SWITCHES = ("G2S_DEVICE_D2", "G2S_RESIDENT", "G2S_D2_BIG", "G2S_D2_NO_CHAINS", "G2S_D2_POLL", "G2S_D2_SMALL_WAVES",
            "G2S_NO_SEG_TIER", "G2S_FORCE_SEGX", "G2S_NO_SEGX_TIER", "G2S_SEG_WAVES")
_DEV = dict(G2S_DEVICE_D2="1", G2S_RESIDENT="1")
# (G2S_D2_SMALL_WAVES is read once per process: its leg is test_small_instantiation_alone, in a child process)
LEGS = {
    "device": _DEV,
    "big-takes-all": dict(_DEV, G2S_D2_BIG="2"),
    "no-chains": dict(_DEV, G2S_D2_NO_CHAINS="1"),
    "poll": dict(_DEV, G2S_D2_POLL="1"),
    "host-threads": dict(G2S_DEVICE_D2="0", G2S_RESIDENT="1"),
    "not-resident": dict(G2S_RESIDENT="0"),
    # the large instantiation behind the small one on every list (by default: on deep lists only), so that the closures
    # of more than 256 segments are the device's on the lists that are not deep too
    "big-behind": dict(_DEV, G2S_D2_BIG="1"),
    "no-chains-big-behind": dict(_DEV, G2S_D2_BIG="1", G2S_D2_NO_CHAINS="1"),
    "poll-big-behind": dict(_DEV, G2S_D2_BIG="1", G2S_D2_POLL="1"),
}
DEEP = 2500  # (g2s_api.hip: a list with a gap of D = lmf + rmf + g + d_err >= 2500 is deep)


def _is_deep(d_err):
    return any(2 * DC.FUZ + DC.design(n)["gap"]["gap_len"] + d_err >= DEEP for n in DC.names_at(d_err))


def _left_to_the_host(d_err, env):
    """The designs the small instantiation passes on with nobody behind it."""
    big = env.get("G2S_D2_BIG")
    follows = (big != "0") if big is not None else _is_deep(d_err)
    return [] if follows else [n for n in DC.names_at(d_err) if DC.takes_big(n)]


@pytest.mark.parametrize("d_err", DC.D_ERRS)
@pytest.mark.parametrize("leg", sorted(LEGS))
def test_designed_components_equal_the_oracle(product, oracle, monkeypatch, leg, d_err):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for kv in LEGS[leg].items():
        monkeypatch.setenv(*kv)
    seqs, gaps, idx, names = DC.design_list(d_err, pad=100)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, d_err)
    assert c == len(gaps)  # (every design and every ordinary gap compared: none is a Q7 case)
    assert tm.watchdog_gaps == 0
    if leg != "not-resident":
        assert tm.resident_launches == 1 and tm.resident_fallbacks == 0
        if leg == "host-threads":
            assert tm.host_finished_gaps >= len(names)
        else:
            assert tm.host_finished_gaps == len(_left_to_the_host(d_err, LEGS[leg]))
    # -best-only: the traceback starts are the sinks, the closure is that of one or two path lengths — still with the
    # cycles' k-mers at several depths (tests/test_d2_cases.py runs the host's phase D on these closures too)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, d_err, False, False)
    assert c == len(gaps) and tm.watchdog_gaps == 0
    if leg != "not-resident":
        assert tm.resident_launches == 1 and tm.resident_fallbacks == 0


def _rows(by, name):
    return [(x["kernel"], x["rc"]) for x in by[name]]


def _report(d_err, by):
    for n, rows in by.items():
        print("-dist-error %d %-20s ncl %4d: %s" % (d_err, n, DC.DESIGNS[n][3]["ncl"], " ".join(
            "(%s rc %d nrec %d ns %d nv %d ne %d)" % ("g2s_d2_big" if x["kernel"] else "g2s_d2_small", x["rc"], x["nrec"], x["ns"],
                                                       x["nv"], x["ne"]) for x in rows)))


@pytest.mark.parametrize("d_err", DC.D_ERRS)
def test_every_design_is_taken_by_a_d2_kernel(product, oracle, tmp_path, d_err):
    """The witness: with the large instantiation behind the small one, every design has a log row with rc == 0 from a
    D2 kernel — no fill kernel analysed it, no host took it —, from g2s_d2_small up to 256 closure segments and, behind
    a row of g2s_d2_small with rc != 0, from g2s_d2_big beyond; the list's results are the oracle's."""
    by, res, tm = d2_log_of_designs(tmp_path, d_err, G2S_D2_BIG="1")
    _report(d_err, by)
    seqs, gaps, idx, names = DC.design_list(d_err, pad=100)
    for n in names:
        rows = _rows(by, n)
        assert any(rc == 0 for _, rc in rows), (n, by[n])
        if DC.takes_big(n):
            assert len(rows) == 2 and rows[0][0] == 0 and rows[0][1] != 0 and rows[1] == (1, 0), (n, by[n])
        else:
            assert rows == [(0, 0)], (n, by[n])
        assert by[n][-1]["ns"] == DC.DESIGNS[n][3]["ncl"], (n, by[n])  # the closure the model and the oracle agree on
    if d_err == 150:  # the ladder of 90 bubbles: passed on by g2s_d2_small, taken by g2s_d2_big
        assert _rows(by, "cycle+bubbles-90")[0][1] != 0 and _rows(by, "cycle+bubbles-90")[1] == (1, 0)
    assert tm.host_finished_gaps == 0
    c, f, _, _, _ = _check_batch(product, oracle, seqs, K, gaps, d_err, run_product=lambda sess, g: (res, tm))
    assert c == len(gaps)


@pytest.mark.parametrize("d_err", DC.D_ERRS)
def test_small_instantiation_alone(product, oracle, tmp_path, d_err):
    """G2S_D2_SMALL_WAVES=1 (g2s_d2_small on one wave a closure) on the library's default otherwise: on a list that is
    not deep no large instantiation follows, the designs of more than 256 closure segments are passed on (rc != 0) and
    finished by the host's threads; on the deep list g2s_d2_big takes them.  The results are the oracle's either way."""
    by, res, tm = d2_log_of_designs(tmp_path, d_err)
    _report(d_err, by)
    seqs, gaps, idx, names = DC.design_list(d_err, pad=100)
    host = _left_to_the_host(d_err, {})
    for n in names:
        rows = _rows(by, n)
        if not DC.takes_big(n):
            assert rows == [(0, 0)], (n, by[n])
        elif n in host:
            assert len(rows) == 1 and rows[0][0] == 0 and rows[0][1] != 0, (n, by[n])
        else:
            assert len(rows) == 2 and rows[0][1] != 0 and rows[1] == (1, 0), (n, by[n])
    assert tm.host_finished_gaps == len(host)
    c, f, _, _, _ = _check_batch(product, oracle, seqs, K, gaps, d_err, run_product=lambda sess, g: (res, tm))
    assert c == len(gaps)
