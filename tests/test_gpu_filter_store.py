"""The store route of the batched read filter's one-pass mode on the MI355X (gap2seq_amd/csrc/bam_store.hip): the store the
kernels write behind the row kernels against the host model (pinned to the format in tests/test_filter_store.py), byte for
byte and offset for offset, at every walk window of the cut files; pass B from the store against the host walk; the
batched filter over the cap of the whole stream, end to end, against the same call with one-pass mode off and with
device -1; the bound's edge, the switches, an overflow of either planned capacity, every other way out, and
Gap2Seq-libraries under the cap."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import bamwriter as BW  # noqa: E402
import bam_store_cases as SC  # noqa: E402
import bam_text_cases as TC  # noqa: E402
import bam_walk_cases as WC  # noqa: E402
import inflate_cases as IC  # noqa: E402
from test_gpu_bam_text import EXE, FORMS, GAPS, _library  # noqa: E402

pytestmark = pytest.mark.gpu

G2S_OK, G2S_ERR_IO = 0, -2
ON_DEVICE, NOT_ASKED, NO_DEVICE_ROWS, OVER_CAP, STORE_OVERFLOW = 0, 1, 2, 3, 5
SWITCHES = ("G2S_HOST_FILTER", "G2S_HOST_INFLATE", "G2S_DEVICE_INFLATE", "G2S_HOST_ROWS", "G2S_DEVICE_ROWS",
            "G2S_FILTER_ONE_PASS", "G2S_FILTER_RESIDENT_CAP", "G2S_FILTER_STORE", "G2S_FILTER_STORE_SAMPLE")
STORE_FILES = (TC.designed(),) + TC.small_files() + tuple(WC.field_cases())
CUT_FILES = {c.name: c for c in TC.window_cases() + tuple(WC.cut_cases())}   # (cut_cases are among window_cases: once each)


@pytest.fixture
def P(product, monkeypatch):
    """the product with no switch set and the mode following the environment, before and after"""
    for k in SWITCHES + ("G2S_BAM_CHUNK",):
        monkeypatch.delenv(k, raising=False)
    product.filter_set_one_pass(-1)
    yield product
    product.filter_set_one_pass(-1)


def _chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("G2S_BAM_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)


# ---- 1. the store against the host model

def _store_equals_model(P, case, windows):
    rc, want, msg = P.bam_store(case.data, device=-1)
    assert rc == G2S_OK, msg
    for window in windows:
        rc, got, msg = P.bam_store(case.data, device=0, window=window)
        assert rc == G2S_OK, (window, msg)
        assert got[1] == want[1], window
        assert got[0] == want[0], window
    return want


@pytest.mark.parametrize("case", STORE_FILES, ids=lambda c: c.name)
def test_device_store_equals_the_host_model(P, case):
    store, offs = _store_equals_model(P, case, case.windows)
    assert len(offs) == len(SC.source_records(case.raw))
    if case.name == "text_designed":
        assert len(store) > 3000 and len(offs) > 30   # (many 64-byte steps, many records)


@pytest.mark.parametrize("name", sorted(CUT_FILES))
def test_cut_and_carried_records_are_stored_whole(P, monkeypatch, name):
    case = CUT_FILES[name]
    _chunk(monkeypatch, case.chunk)
    if case.chunk and len(case.raw) > WC.FIRST + case.chunk:
        assert len(IC.split_members(case.data)) > 2   # (more than one reader window: records carried in front of a slot)
    _store_equals_model(P, case, case.windows)


# ---- 2. pass B from the store

@pytest.mark.parametrize("name", ["text_designed"] + sorted(c.name for c in TC.window_cases()))
def test_pass_b_from_the_store_equals_the_host_walk(P, monkeypatch, name):
    case = TC.designed() if name == "text_designed" else CUT_FILES[name]
    _chunk(monkeypatch, case.chunk)
    n = len(TC.records(case.raw))
    for what, rows in TC.selections(n):
        for names, fasta in FORMS:
            rc, want, msg = P.bam_text(case.data, rows, device=-1, names=names, fasta=fasta)
            assert rc == G2S_OK, msg
            # every selection and form at the case's smallest walk window, every row at each of the others
            for window in (case.windows if what == "all" else case.windows[-1:]):
                rc, got, msg = P.bam_text(case.data, rows, device=0, names=names, fasta=fasta, store=True, window=window)
                assert rc == G2S_OK, (what, names, fasta, window, msg)
                assert got == want, (what, names, fasta, window)


# ---- 3. the batched filter over the whole stream's cap, end to end

def _calls(P, bam, gaps, device=0):
    """every form of the batched call, and what the hooks said after each"""
    out, hooks = [], []

    def note(stats):
        hooks.append((stats["file_passes"], P.last_filter_text(), P.last_filter_inflate(), P.last_filter_store()))

    texts, stats, un = P.filter_reads_gaps(bam, 300, 20, gaps, device=device, unmapped=True)
    note(stats)
    out += [texts, un]
    texts, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=device)
    note(stats)
    out.append(texts)
    for names, unmapped in ((True, True), (True, False), (False, True), (False, False)):
        pool = P.filter_reads_gaps_pool(bam, 300, 20, gaps, device=device, names=names, unmapped=unmapped)
        note(pool.stats)
        out.append((pool.seqs, pool.names, [list(pool.gap_reads(i)) for i in range(len(gaps))], list(pool.unmapped),
                    pool.n_reads, pool.total))
        pool.free()
    return out, hooks


def _raw(P, bam):
    rc, raw, _, _ = P.bgzf_inflate(bam, -1)
    assert rc == G2S_OK
    return raw


def _whole_need(raw):
    return len(raw) + 52 * (len(raw) // 36 + 1)


@pytest.mark.parametrize("chunk", [None, "windows"], ids=["one_window", "six_windows"])
def test_over_the_cap_the_store_route_takes_one_pass(P, monkeypatch, chunk):
    """(on the parent commit these calls take two passes with reason 3)"""
    bam, gaps, n_records = _library()
    raw = _raw(P, bam)
    assert (len(raw), n_records, _whole_need(raw)) == (747241, 6080, 1826605)
    cap = _whole_need(raw) - 1
    monkeypatch.setenv("G2S_FILTER_RESIDENT_CAP", str(cap))
    _chunk(monkeypatch, len(raw) // 6 if chunk else None)
    P.filter_set_one_pass(1)
    one, hooks = _calls(P, bam, gaps)
    for passes, text, inflate, store in hooks:
        print(passes, text, inflate, store)
        assert passes == 1
        assert (text["one_pass"], text["reason"]) == (1, ON_DEVICE) and 0 < text["resident_bytes"] < len(raw)
        assert (store["used"], store["overflow"], store["records"]) == (1, 0, n_records)
        assert store["store_bytes"] == text["resident_bytes"] <= store["store_cap"] and n_records <= store["rows_cap"]
        assert store["device_bytes"] <= cap
        assert inflate["on_device"] == 1 and inflate["bytes_out"] == len(raw)   # (once)
    assert P.last_filter_rows()["records"] == n_records
    P.filter_set_one_pass(0)
    two, hooks = _calls(P, bam, gaps)
    for passes, text, inflate, store in hooks:
        assert passes == 2 and (text["one_pass"], text["reason"], text["resident_bytes"]) == (0, NOT_ASKED, 0)
        assert (store["used"], store["store_cap"]) == (0, 0) and inflate["bytes_out"] == 2 * len(raw)
    host, _ = _calls(P, bam, gaps, device=-1)
    assert one == two
    assert one == host
    assert sum(x[3] for x in one[0]) > 100 and one[1][3] == 210   # (the gaps select reads, and the unmapped reads are there)


# ---- 4. the bound's edge

def test_the_route_is_taken_at_its_need_and_not_a_byte_below(P, monkeypatch):
    bam, gaps, n_records = _library()
    rc, plan, msg = P.filter_store_plan(bam)
    assert rc == G2S_OK and plan["need"] < _whole_need(_raw(P, bam)), msg
    P.filter_set_one_pass(1)
    monkeypatch.setenv("G2S_FILTER_RESIDENT_CAP", str(plan["need"]))
    at, stats, un_at = P.filter_reads_gaps(bam, 300, 20, gaps, device=0, unmapped=True)
    text, store = P.last_filter_text(), P.last_filter_store()
    assert (stats["file_passes"], text["one_pass"], text["reason"]) == (1, 1, ON_DEVICE)
    assert (store["used"], store["overflow"], store["records"]) == (1, 0, n_records)
    assert (store["device_bytes"], store["rows_cap"], store["store_cap"]) == (plan["need"], plan["rows_cap"], plan["store_cap"])
    monkeypatch.setenv("G2S_FILTER_RESIDENT_CAP", str(plan["need"] - 1))
    below, stats, un_below = P.filter_reads_gaps(bam, 300, 20, gaps, device=0, unmapped=True)
    text, store = P.last_filter_text(), P.last_filter_store()
    assert (stats["file_passes"], text["one_pass"], text["reason"], text["resident_bytes"]) == (2, 0, OVER_CAP, 0)
    assert (store["used"], store["overflow"]) == (0, 0)
    assert (at, un_at) == (below, un_below) and sum(x[3] for x in at) > 100


# ---- 5. the switches

def test_the_switch_takes_the_route_or_forbids_it(P, monkeypatch):
    bam, gaps, n_records = _library()
    raw = _raw(P, bam)
    P.filter_set_one_pass(1)
    plain, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    text = P.last_filter_text()
    assert (stats["file_passes"], text["reason"]) == (1, ON_DEVICE) and text["resident_bytes"] >= len(raw)
    assert P.last_filter_store()["used"] == 0
    monkeypatch.setenv("G2S_FILTER_STORE", "1")   # (no cap: the stream would fit)
    forced, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    text, store = P.last_filter_text(), P.last_filter_store()
    assert (stats["file_passes"], text["one_pass"], text["reason"]) == (1, 1, ON_DEVICE) and 0 < text["resident_bytes"] < len(raw)
    assert (store["used"], store["overflow"], store["records"]) == (1, 0, n_records)
    monkeypatch.setenv("G2S_FILTER_STORE", "0")
    monkeypatch.setenv("G2S_FILTER_RESIDENT_CAP", str(_whole_need(raw) - 1))
    never, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    text, store = P.last_filter_text(), P.last_filter_store()
    assert (stats["file_passes"], text["one_pass"], text["reason"], text["resident_bytes"]) == (2, 0, OVER_CAP, 0)
    assert (store["used"], store["store_cap"]) == (0, 0)
    assert plain == forced == never


# ---- 6. a planned capacity that proves too small

@pytest.mark.parametrize("which", [1, 2], ids=["rows", "store"])
def test_an_overflow_starts_over_and_returns_the_same_bytes(P, monkeypatch, which):
    case = SC.rows_overflow() if which == 1 else SC.store_overflow()
    monkeypatch.setenv("G2S_FILTER_STORE_SAMPLE", str(SC.OVERFLOW_SAMPLE))
    rc, plan, msg = P.filter_store_plan(case.data)
    assert rc == G2S_OK, msg
    store, offs = SC.compact(case.raw)
    assert (len(offs) > plan["rows_cap"], len(store) > plan["store_cap"]) == (which == 1, which == 2)   # that one, and only that one
    P.filter_set_one_pass(0)
    plain, _ = _calls(P, case.data, GAPS)
    monkeypatch.setenv("G2S_FILTER_STORE", "1")
    P.filter_set_one_pass(1)
    asked, hooks = _calls(P, case.data, GAPS)
    for passes, text, inflate, hook in hooks:
        assert passes == 3 and (text["one_pass"], text["reason"], text["resident_bytes"]) == (0, STORE_OVERFLOW, 0)
        assert (hook["used"], hook["overflow"]) == (0, which)
        assert (hook["rows_cap"], hook["store_cap"]) == (plan["rows_cap"], plan["store_cap"])
    assert asked == plain
    assert sum(x[3] for x in plain[0]) > 0
    rows = P.last_filter_rows()
    assert (rows["on_device"], rows["anomaly"], rows["records"]) == (1, 0, len(offs))   # (pass A's second run: the kernels again)


# ---- 7. every other way out

@pytest.mark.parametrize("case", WC.handed_over_cases(), ids=lambda c: c.name)
def test_a_pass_a_anomaly_takes_two_passes_in_store_form(P, monkeypatch, case):
    _chunk(monkeypatch, case.chunk)
    P.filter_set_one_pass(0)
    plain, _ = _calls(P, case.data, GAPS)
    monkeypatch.setenv("G2S_FILTER_STORE", "1")
    P.filter_set_one_pass(1)
    asked, hooks = _calls(P, case.data, GAPS)
    assert asked == plain
    for passes, text, inflate, store in hooks:
        assert passes == 2 and (text["one_pass"], text["reason"]) == (0, NO_DEVICE_ROWS)
        assert (store["used"], store["overflow"]) == (0, 0)
        assert inflate["bytes_out"] == 2 * len(case.raw)
    hook = P.last_filter_rows()
    assert (hook["on_device"], hook["anomaly"]) == (0, case.anomaly)


@pytest.mark.parametrize("case", WC.error_cases(), ids=lambda c: c[0])
def test_broken_files_give_the_host_message_in_store_form(P, monkeypatch, case):
    _, data, chunk, message = case
    _chunk(monkeypatch, chunk)
    seen = []
    for mode, store in ((0, None), (1, "1")):
        P.filter_set_one_pass(mode)
        if store:
            monkeypatch.setenv("G2S_FILTER_STORE", store)
        for call in (P.filter_reads_gaps, P.filter_reads_gaps_pool):
            with pytest.raises(P.G2SError) as e:
                call(data, 300, 20, GAPS, device=0)
            seen.append((e.value.code, str(e.value)))
            assert P.last_filter_text()["one_pass"] == 0 and P.last_filter_store()["used"] == 0
    assert all(code == G2S_ERR_IO and message in msg for code, msg in seen), seen
    assert len(set(seen)) == 1


# ---- 8. Gap2Seq-libraries

def test_libraries_output_under_the_cap_does_not_depend_on_the_route(P, tmp_path):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    K, FUZ, length = 31, 10, 6000
    rng = random.Random(29)
    genome = "".join(rng.choice("ACGT") for _ in range(length))  # (simulate_library's first draws)
    lines, whole, needs = [], [], []
    for i, (pairs, mean, sd, thr) in enumerate([(900, 300, 20, 0.0), (700, 250, 30, 0.5)]):   # (one cap has to serve both files)
        refs, recs, _ = BW.simulate_library(29, n_scaffolds=1, scaffold_len=length, gap=(3000, 200), pairs=pairs, mean=mean,
                                            sd=sd, unmapped_pairs=10, ambiguous=0.0)
        bam = BW.bam_bytes(refs, recs, block=[65280, 700][i])
        (tmp_path / ("lib%d.bam" % i)).write_bytes(bam)
        lines.append("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), mean, sd, thr))
        whole.append(_whole_need(_raw(P, bam)))
        needs.append(P.filter_store_plan(bam)[1]["need"])
    cap = min(whole) - 1   # under either file's whole stream, over either file's store
    assert max(needs) <= cap
    fl = K + FUZ
    records, bed = [], []
    for j, (bp, gl) in enumerate([(3000, 200), (700, 100), (2200, 150), (4600, 80)]):
        records.append(">scaf0 scaffold 0 contig %d gap %d\n%s\n" % (j, j, genome[bp - fl:bp] + "N" * gl + genome[bp + gl:bp + gl + fl]))
        bed.append("scaf0\t%d\t%d\n" % (bp - fl, bp + gl + fl))
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join(lines))
    outs = []
    for mode in ("1", "0"):  # (G2S_DEBUG=1: the library says on stderr which route every file took)
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e["G2S_DEBUG"] = "1"
        e["G2S_FILTER_RESIDENT_CAP"] = str(cap)
        out = tmp_path / (mode + ".fa")
        run = subprocess.run([EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                              str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(K), "-fuz", str(FUZ), "-solid", "1",
                              "-dist-error", "100", "-randseed", "3", "-filter-one-pass", mode],
                             capture_output=True, text=True, timeout=300, env=e)
        assert run.returncode == 0, run.stderr
        assert run.stderr.count("heads, names and bases stay on the device") == (2 if mode == "1" else 0), run.stderr
        assert "the inflated file stays on the device" not in run.stderr and "given up" not in run.stderr, run.stderr
        outs.append((out.read_bytes(), run.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert b">" in outs[0][0]
