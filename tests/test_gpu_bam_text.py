"""Pass B of the batched read filter on the MI355X (gap2seq_amd/csrc/bam_text.hip) and one-pass mode: the designed records
of tests/bam_text_cases.py and the cut files of tests/bam_walk_cases.py through the kernels against the host walk, array
for array; the batched filter with one-pass mode on against the same call with it off and with device -1, byte for byte;
every way out of one-pass mode; and Gap2Seq-libraries with -filter-one-pass 1 against 0."""
import functools
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import bamwriter as BW  # noqa: E402
import bam_text_cases as TC  # noqa: E402
import bam_walk_cases as WC  # noqa: E402
import inflate_cases as IC  # noqa: E402

pytestmark = pytest.mark.gpu

G2S_OK, G2S_ERR_IO = 0, -2
ON_DEVICE, NOT_ASKED, NO_DEVICE_ROWS, OVER_CAP = 0, 1, 2, 3
EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")
SWITCHES = ("G2S_HOST_FILTER", "G2S_HOST_INFLATE", "G2S_DEVICE_INFLATE", "G2S_HOST_ROWS", "G2S_DEVICE_ROWS",
            "G2S_FILTER_ONE_PASS", "G2S_FILTER_RESIDENT_CAP")
GAPS = [("scaf0", 500, 100, 50), ("scaf1", 300, 10, -1), ("scaf2", 6050, 30, 40), ("nosuch", 10, 5, 5)]
FILES = (TC.designed(),) + TC.small_files()
FORMS = ((True, False), (False, False), (False, True))   # (names, fasta)


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


# ---- the kernels on the designed records

@pytest.mark.parametrize("case", FILES, ids=lambda c: c.name)
def test_device_text_equals_the_host_walk(P, case):
    n = len(TC.records(case.raw))
    for what, rows in TC.selections(n):
        for names, fasta in FORMS:
            rc, want, msg = P.bam_text(case.data, rows, device=-1, names=names, fasta=fasta)
            assert rc == G2S_OK, msg
            rc, got, msg = P.bam_text(case.data, rows, device=0, names=names, fasta=fasta)
            assert rc == G2S_OK, (what, names, fasta, msg)
            assert got == want, (what, names, fasta)
            if what == "all" and n > 1:
                assert len(want["bases"]) > 3000 and len(want["base_off"]) == n + 1   # (many 64-byte steps, many records)


# ---- records cut by windows of the resident stream

@pytest.mark.parametrize("case", TC.window_cases(), ids=lambda c: c.name)
def test_cut_records_are_whole_in_the_resident_stream(P, monkeypatch, case):
    _chunk(monkeypatch, case.chunk)
    rows = list(range(len(TC.records(case.raw))))
    if case.chunk and len(case.raw) > WC.FIRST + case.chunk:
        assert len(IC.split_members(case.data)) > 2   # (more than one reader window)
    for names, fasta in ((True, False), (False, True)):
        rc, want, msg = P.bam_text(case.data, rows, device=-1, names=names, fasta=fasta)
        assert rc == G2S_OK, msg
        rc, got, msg = P.bam_text(case.data, rows, device=0, names=names, fasta=fasta)
        assert rc == G2S_OK, msg
        assert got == want
    # pass A in one-pass mode makes the rows the host walk makes, array for array, at every walk window too
    rc, want_rows, msg = P.bam_rows(case.data, -1)
    assert rc == G2S_OK, msg
    for window in case.windows:
        rc, got_rows, msg = P.bam_rows(case.data, 0, window, kept=True)
        assert rc == G2S_OK, (window, msg)
        assert got_rows == want_rows, window
        hook = P.last_filter_rows()
        assert (hook["on_device"], hook["anomaly"], hook["records"]) == (1, 0, want_rows["total"])
    P.filter_set_one_pass(1)
    texts, stats = P.filter_reads_gaps(case.data, 300, 20, GAPS, device=0)
    hook, rows_hook = P.last_filter_text(), P.last_filter_rows()
    assert (stats["file_passes"], hook["one_pass"], hook["resident_bytes"]) == (1, 1, len(case.raw))
    assert (rows_hook["on_device"], rows_hook["anomaly"], rows_hook["records"]) == (1, 0, len(rows))
    P.filter_set_one_pass(0)
    assert P.filter_reads_gaps(case.data, 300, 20, GAPS, device=0)[0] == texts


# ---- the batched filter, end to end

@functools.lru_cache(maxsize=None)
def _library():
    """the 1 500-pair library of tests/test_gpu_bam_rows.py, its 42 gaps, and a gap named three times"""
    refs, recs, _ = BW.simulate_library(43, n_scaffolds=2, scaffold_len=12000, gap=(6000, 250), pairs=1500, unmapped_pairs=40)
    rng = random.Random(44)
    gaps = [(rng.choice(refs)[0], rng.randrange(500, 11500), rng.choice([-1, 0, rng.randrange(1, 400)]),
             rng.choice([-1, 0, rng.randrange(1, 150)])) for _ in range(40)] + [("scaf0", 6000, 250, 60), ("nosuch", 10, 5, 5)]
    gaps += [("scaf0", 6000, 250, 60), ("scaf0", 6010, 250, 300)]
    return BW.bam_bytes(refs, recs, block=5000), gaps, len(recs)


def _calls(P, bam, gaps, device=0):
    """every form of the batched call, and what the hooks said after each"""
    out, hooks = [], []

    def note(stats):
        hooks.append((stats["file_passes"], P.last_filter_text(), P.last_filter_inflate()))

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


def _one_pass_equals_two_pass(P, bam, gaps, raw_len):
    P.filter_set_one_pass(1)
    one, hooks = _calls(P, bam, gaps)
    for passes, text, inflate in hooks:
        assert passes == 1
        assert (text["one_pass"], text["reason"]) == (1, ON_DEVICE) and text["resident_bytes"] >= raw_len
        assert inflate["on_device"] == 1 and inflate["bytes_out"] == raw_len
        assert inflate["members"] == len(IC.split_members(bam))
    P.filter_set_one_pass(0)
    two, hooks = _calls(P, bam, gaps)
    for passes, text, inflate in hooks:
        assert passes == 2 and (text["one_pass"], text["reason"], text["resident_bytes"]) == (0, NOT_ASKED, 0)
        assert inflate["bytes_out"] == 2 * raw_len
    host, _ = _calls(P, bam, gaps, device=-1)
    assert one == two
    assert one == host
    return one, hooks


@pytest.mark.parametrize("chunk", [None, "windows"], ids=["one_window", "six_windows"])
def test_one_pass_returns_the_bytes_of_two_passes(P, monkeypatch, chunk):
    bam, gaps, n_records = _library()
    rc, raw, _, _ = P.bgzf_inflate(bam, -1)
    assert rc == G2S_OK and len(raw) > 300000
    _chunk(monkeypatch, len(raw) // 6 if chunk else None)
    one, _ = _one_pass_equals_two_pass(P, bam, gaps, len(raw))
    assert P.last_filter_rows()["records"] == n_records
    texts, un, pool = one[0], one[1], one[3]
    assert sum(x[3] for x in texts) > 100 and un[3] == 210
    seqs, names, gap_reads, unmapped, n_reads, total = pool
    assert total == n_records and n_reads < sum(len(g) for g in gap_reads) + len(unmapped)
    # what the gap list is for: a read several gaps select, a read twice in one gap (its lists 1 and 2), unmapped reads
    # that a gap selects too, and gaps that select nothing
    assert gap_reads[40] == gap_reads[42] and gap_reads[40]
    assert any(len(set(g)) < len(g) for g in gap_reads)
    assert set(unmapped) & {r for g in gap_reads for r in g}
    assert gap_reads[41] == [] and texts[41][3] == 0


def test_one_pass_with_no_selection_and_with_no_gaps(P):
    bam, _, n_records = _library()
    rc, raw, _, _ = P.bgzf_inflate(bam, -1)
    for gaps in ([("nosuch", 10, 5, 5), ("scaf0", 11990, -1, -1)], []):
        one, _ = _one_pass_equals_two_pass(P, bam, gaps, len(raw))
        assert all(x[3] == 0 for x in one[0]) and one[1][3] == 210
        assert one[3][4] == 210 and one[4][4] == 0   # the pool: the unmapped reads alone, or nothing


# ---- every way out of one-pass mode

def _asked_equals_plain(P, data, gaps=GAPS):
    P.filter_set_one_pass(0)
    plain, _ = _calls(P, data, gaps)
    P.filter_set_one_pass(1)
    asked, hooks = _calls(P, data, gaps)
    assert asked == plain
    return hooks


def test_over_the_cap_takes_two_passes(P, monkeypatch):
    bam, gaps, _ = _library()
    monkeypatch.setenv("G2S_FILTER_RESIDENT_CAP", "1")
    for passes, text, inflate in _asked_equals_plain(P, bam, gaps):
        assert passes == 2 and (text["one_pass"], text["reason"], text["resident_bytes"]) == (0, OVER_CAP, 0)
        assert inflate["on_device"] == 1
    assert P.last_filter_rows()["on_device"] == 1   # (pass A's rows are still the kernels')


def test_the_environment_asks_on_the_device_too(P, monkeypatch):
    bam, gaps, _ = _library()
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "1")
    _, stats = P.filter_reads_gaps(bam, 300, 20, gaps[:3], device=0)
    assert stats["file_passes"] == 1 and P.last_filter_text()["one_pass"] == 1
    monkeypatch.setenv("G2S_FILTER_ONE_PASS", "0")
    _, stats = P.filter_reads_gaps(bam, 300, 20, gaps[:3], device=0)
    assert stats["file_passes"] == 2 and P.last_filter_text()["reason"] == NOT_ASKED


@pytest.mark.parametrize("switch", ["G2S_HOST_ROWS", "G2S_HOST_INFLATE", "G2S_HOST_FILTER"])
def test_switches_that_keep_pass_a_on_the_host_take_two_passes(P, monkeypatch, switch):
    bam, gaps, _ = _library()
    monkeypatch.setenv(switch, "1")
    for passes, text, _ in _asked_equals_plain(P, bam, gaps[:6]):
        assert passes == 2 and (text["one_pass"], text["reason"], text["resident_bytes"]) == (0, NO_DEVICE_ROWS, 0)


@pytest.mark.parametrize("case", WC.handed_over_cases(), ids=lambda c: c.name)
def test_a_pass_a_anomaly_takes_two_passes(P, monkeypatch, case):
    _chunk(monkeypatch, case.chunk)
    for passes, text, inflate in _asked_equals_plain(P, case.data):
        assert passes == 2 and (text["one_pass"], text["reason"]) == (0, NO_DEVICE_ROWS)
        assert inflate["bytes_out"] == 2 * len(case.raw)
    hook = P.last_filter_rows()
    assert (hook["on_device"], hook["anomaly"]) == (0, case.anomaly)


@pytest.mark.parametrize("case", WC.error_cases(), ids=lambda c: c[0])
def test_broken_files_give_the_host_message_in_one_pass_mode(P, monkeypatch, case):
    _, data, chunk, text = case
    _chunk(monkeypatch, chunk)
    seen = []
    for mode in (1, 0):
        P.filter_set_one_pass(mode)
        for call in (P.filter_reads_gaps, P.filter_reads_gaps_pool):
            with pytest.raises(P.G2SError) as e:
                call(data, 300, 20, GAPS, device=0)
            seen.append((e.value.code, str(e.value)))
            assert P.last_filter_text()["one_pass"] == 0
    assert all(code == G2S_ERR_IO and text in msg for code, msg in seen), seen
    assert len(set(seen)) == 1


# ---- Gap2Seq-libraries

def test_libraries_output_does_not_depend_on_the_number_of_passes(tmp_path):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    K, FUZ, length = 31, 10, 6000
    rng = random.Random(29)
    genome = "".join(rng.choice("ACGT") for _ in range(length))  # (simulate_library's first draws)
    lines = []
    for i, (pairs, mean, sd, thr) in enumerate([(900, 300, 20, 0.0), (400, 250, 30, 0.5)]):
        refs, recs, _ = BW.simulate_library(29, n_scaffolds=1, scaffold_len=length, gap=(3000, 200), pairs=pairs, mean=mean,
                                            sd=sd, unmapped_pairs=10, ambiguous=0.0)
        (tmp_path / ("lib%d.bam" % i)).write_bytes(BW.bam_bytes(refs, recs, block=[65280, 700][i]))
        lines.append("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), mean, sd, thr))
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
        out = tmp_path / (mode + ".fa")
        run = subprocess.run([EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                              str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(K), "-fuz", str(FUZ), "-solid", "1",
                              "-dist-error", "100", "-randseed", "3", "-filter-one-pass", mode],
                             capture_output=True, text=True, timeout=300, env=e)
        assert run.returncode == 0, run.stderr
        assert (run.stderr.count("one-pass route: the inflated file stays on the device") == 2) == (mode == "1"), run.stderr
        assert "one-pass route" in run.stderr if mode == "1" else "one-pass route" not in run.stderr, run.stderr
        assert "given up" not in run.stderr, run.stderr
        outs.append((out.read_bytes(), run.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert b">" in outs[0][0]
