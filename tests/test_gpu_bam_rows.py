"""Pass A of the batched read filter on the MI355X (gap2seq_amd/csrc/bam_rows.hip): the designed files of
tests/bam_walk_cases.py through the kernels against the host walk, array for array, at the reader's window and at walk
windows small enough that every cut occurs; the files the kernels must hand over to the host walk; the files the host
walk rejects; and the batched filter and Gap2Seq-libraries with device rows against G2S_HOST_ROWS=1, byte for byte."""
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
import bam_walk_cases as WC  # noqa: E402
import inflate_cases as IC  # noqa: E402

pytestmark = pytest.mark.gpu

G2S_OK, G2S_ERR_IO, G2S_ERR_HIP = 0, -2, -4
EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")
SWITCHES = ("G2S_HOST_FILTER", "G2S_HOST_INFLATE", "G2S_DEVICE_INFLATE", "G2S_HOST_ROWS", "G2S_DEVICE_ROWS")
GAPS = [("scaf0", 500, 100, 50), ("scaf1", 300, 10, -1), ("scaf2", 6050, 30, 40), ("nosuch", 10, 5, 5)]


def _rows(monkeypatch, on):
    """the switches: device rows (forced, whatever the default is), or the host walk with inflate and joins on the device"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("G2S_DEVICE_INFLATE", "1")
    monkeypatch.setenv("G2S_DEVICE_ROWS" if on else "G2S_HOST_ROWS", "1")


def _chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("G2S_BAM_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)


@functools.lru_cache(maxsize=None)
def _host_rows(name):
    """the reference, once a case: the host walk (pinned to a Python parse in tests/test_bam_rows.py)"""
    from gap2seq_amd import lib
    case = {c.name: c for c in WC.designed_cases() + WC.handed_over_cases()}[name]
    rc, rows, msg = lib.bam_rows(case.data, -1)
    assert rc == G2S_OK, msg
    return rows


# ---- the kernels on the designed files

@pytest.mark.parametrize("case", WC.designed_cases(), ids=lambda c: c.name)
def test_device_rows_equal_the_host_walk(product, monkeypatch, case):
    _chunk(monkeypatch, case.chunk)
    want = _host_rows(case.name)
    for window in case.windows:
        rc, rows, msg = product.bam_rows(case.data, 0, window)
        assert rc == G2S_OK, (window, msg)
        assert rows == want, window
        hook = product.last_filter_rows()
        assert (hook["on_device"], hook["anomaly"], hook["records"]) == (1, 0, want["total"]), window
        assert hook["candidates"] >= want["total"]
        if window and want["total"] > 2:
            assert hook["windows"] > 1, window


def test_a_window_of_more_than_one_tile_of_candidates(product, monkeypatch):
    monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)
    case = {c.name: c for c in WC.designed_cases()}["records_4097"]
    rc, rows, _ = product.bam_rows(case.data, 0, 0)
    hook = product.last_filter_rows()
    assert rc == G2S_OK and hook["windows"] == 1 and hook["candidates"] > 4096 and len(case.raw) > 16 * 4096


def test_false_heads_are_candidates_and_no_rows(product, monkeypatch):
    monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)
    case = {c.name: c for c in WC.designed_cases()}["false_starts_in_a_row"]
    rc, rows, _ = product.bam_rows(case.data, 0, 0)
    hook = product.last_filter_rows()
    assert rc == G2S_OK and rows["total"] == 6 and hook["candidates"] >= 6 + 40


# ---- anomalies hand pass A to the host walk

@pytest.mark.parametrize("case", WC.handed_over_cases(), ids=lambda c: c.name)
def test_anomaly_hands_over_to_the_host_walk(product, monkeypatch, case):
    _chunk(monkeypatch, case.chunk)
    for window in case.windows:  # the hook: an error, never the host in the kernels' place
        rc, rows, msg = product.bam_rows(case.data, 0, window)
        assert (rc, rows) == (G2S_ERR_HIP, None), msg
        assert product.last_filter_rows()["anomaly"] == case.anomaly
    out = []
    for on in (True, False):
        _rows(monkeypatch, on)
        texts, stats, un = product.filter_reads_gaps(case.data, 300, 20, GAPS, device=0, unmapped=True)
        hook, inflate = product.last_filter_rows(), product.last_filter_inflate()
        assert (hook["on_device"], hook["anomaly"]) == (0, case.anomaly if on else 0)
        out.append((texts, un, stats["file_passes"], stats["on_device"], inflate["on_device"], inflate["members"],
                    inflate["bytes_in"], inflate["bytes_out"]))
    assert out[0] == out[1]
    assert out[0][4] == 1 and out[0][7] == 2 * len(case.raw)


def test_only_the_listed_cases_hand_over(product, monkeypatch):
    seen = set()
    for case in WC.designed_cases() + WC.handed_over_cases():
        _chunk(monkeypatch, case.chunk)
        for window in case.windows:
            product.bam_rows(case.data, 0, window)
            if product.last_filter_rows()["anomaly"]:
                seen.add(case.name)
    assert seen == {"carry_longer_than_the_front", "name_without_its_nul", "more_candidates_than_the_capacity"}


# ---- errors read the same

@pytest.mark.parametrize("case", WC.error_cases(), ids=lambda c: c[0])
def test_broken_files_give_the_host_message(product, monkeypatch, case):
    _, data, chunk, text = case
    _chunk(monkeypatch, chunk)
    seen = []
    for on in (True, False):
        _rows(monkeypatch, on)
        for call in (product.filter_reads_gaps, product.filter_reads_gaps_pool):
            with pytest.raises(product.G2SError) as e:
                call(data, 300, 20, GAPS, device=0)
            seen.append((e.value.code, str(e.value)))
            hook = product.last_filter_rows()
            assert hook["on_device"] == 0 and (hook["anomaly"] != 0) == on
            assert product.last_filter_inflate()["on_device"] == 1
    assert all(code == G2S_ERR_IO and text in msg for code, msg in seen), seen
    assert len(set(seen)) == 1


# ---- the batched filter, end to end

@functools.lru_cache(maxsize=None)
def _library():
    refs, recs, _ = BW.simulate_library(43, n_scaffolds=2, scaffold_len=12000, gap=(6000, 250), pairs=1500, unmapped_pairs=40)
    rng = random.Random(44)
    gaps = [(rng.choice(refs)[0], rng.randrange(500, 11500), rng.choice([-1, 0, rng.randrange(1, 400)]),
             rng.choice([-1, 0, rng.randrange(1, 150)])) for _ in range(40)] + [("scaf0", 6000, 250, 60), ("nosuch", 10, 5, 5)]
    return BW.bam_bytes(refs, recs, block=5000), gaps, len(recs)


def _both(product, bam, gaps):
    texts, stats, un = product.filter_reads_gaps(bam, 300, 20, gaps, device=0, unmapped=True)
    rows, inflate = product.last_filter_rows(), product.last_filter_inflate()
    pool = product.filter_reads_gaps_pool(bam, 300, 20, gaps, device=0)
    rows_pool = product.last_filter_rows()
    got = (texts, un, [pool.fasta(i) for i in range(len(gaps))], pool.unmapped_fasta(), pool.n_reads, pool.total,
           stats["file_passes"], pool.stats["file_passes"], stats["on_device"], pool.stats["on_device"])
    pool.free()
    figures = {k: inflate[k] for k in ("on_device", "members", "bytes_in", "bytes_out")}
    return got, rows, rows_pool, figures


@pytest.mark.parametrize("chunk", [None, "windows"], ids=["one_window", "six_windows"])
def test_filter_with_device_rows_equals_host_rows(product, monkeypatch, chunk):
    bam, gaps, n_records = _library()
    rc, raw, _, _ = product.bgzf_inflate(bam, -1)
    assert rc == G2S_OK and len(raw) > 300000
    _chunk(monkeypatch, len(raw) // 6 if chunk else None)
    _rows(monkeypatch, True)
    dev, dev_rows, dev_rows_pool, dev_figures = _both(product, bam, gaps)
    _rows(monkeypatch, False)
    host, host_rows, _, host_figures = _both(product, bam, gaps)
    for hook in (dev_rows, dev_rows_pool):
        assert (hook["on_device"], hook["anomaly"], hook["records"]) == (1, 0, n_records)
        assert hook["windows"] >= (6 if chunk else 1)
    assert (host_rows["on_device"], host_rows["anomaly"], host_rows["records"]) == (0, 0, n_records)
    assert dev_figures == host_figures
    assert dev_figures["on_device"] == 1 and dev_figures["bytes_out"] == 2 * len(raw)
    assert dev_figures["members"] == 2 * len(IC.split_members(bam))
    assert dev == host
    assert sum(x[3] for x in dev[0]) > 100


def test_switches_that_keep_the_rows_on_the_host(product, monkeypatch):
    bam, gaps, n_records = _library()
    for switch in ("G2S_HOST_ROWS", "G2S_HOST_INFLATE", "G2S_HOST_FILTER"):
        _rows(monkeypatch, True)
        monkeypatch.setenv(switch, "1")
        product.filter_reads_gaps(bam, 300, 20, gaps[:3], device=0)
        hook = product.last_filter_rows()
        assert (hook["on_device"], hook["anomaly"], hook["records"]) == (0, 0, n_records), switch
    _rows(monkeypatch, True)
    product.filter_reads_gaps(bam, 300, 20, gaps[:3], device=-1)
    assert product.last_filter_rows()["on_device"] == 0


# ---- Gap2Seq-libraries

def test_libraries_output_does_not_depend_on_where_the_rows_are_made(tmp_path):
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
    # (G2S_DEBUG=1: the library says on stderr where each file's rows were made)
    for name, env in (("dev", {"G2S_DEVICE_ROWS": "1", "G2S_DEBUG": "1"}), ("host", {"G2S_HOST_ROWS": "1", "G2S_DEBUG": "1"})):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        out = tmp_path / (name + ".fa")
        run = subprocess.run([EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                              str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(K), "-fuz", str(FUZ), "-solid", "1",
                              "-dist-error", "100", "-randseed", "3"], capture_output=True, text=True, timeout=300, env=e)
        assert run.returncode == 0, run.stderr
        # rows on the device in the one child and not in the other, and no quiet hand-over in either
        assert "no device rows" not in run.stderr, run.stderr
        assert ("pass A: rows on the device" in run.stderr) == (name == "dev"), run.stderr
        outs.append((out.read_bytes(), run.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert b">" in outs[0][0]
