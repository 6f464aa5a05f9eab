"""BGZF members inflated on the MI355X (gap2seq_amd/csrc/bgzf_inflate.hip): the designed and corrupt members of
tests/inflate_cases.py through the kernel, and the batched read filter and Gap2Seq-libraries with the reader inflating
on the device against the same calls with G2S_HOST_INFLATE=1, byte for byte."""
import functools
import os
import random
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import bamwriter as BW  # noqa: E402
import inflate_cases as IC  # noqa: E402

pytestmark = pytest.mark.gpu

G2S_OK, G2S_ERR_IO = 0, -2
EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")


def _device_inflate(monkeypatch, on):
    """the reader's switches: the device (forced, whatever the default is) or zlib with the joins still on the device"""
    monkeypatch.delenv("G2S_HOST_FILTER", raising=False)
    if on:
        monkeypatch.delenv("G2S_HOST_INFLATE", raising=False)
        monkeypatch.setenv("G2S_DEVICE_INFLATE", "1")
    else:
        monkeypatch.setenv("G2S_HOST_INFLATE", "1")


# ---- the kernel on the designed members

def test_valid_members_as_one_file(product):
    for eof in (True, False):
        data, payload = IC.valid_file(eof)
        rc, got, bad, msg = product.bgzf_inflate(data, 0)
        assert rc == G2S_OK, msg
        assert got == payload
    one = IC.valid_cases()[0]
    assert product.bgzf_inflate(one[1], 0)[:2] == (G2S_OK, one[2])


def test_valid_members_in_several_windows(product, monkeypatch):
    data, payload = IC.valid_file()
    monkeypatch.setenv("G2S_BAM_CHUNK", "70000")
    rc, got, _, msg = product.bgzf_inflate(data, 0)
    assert rc == G2S_OK, msg
    assert got == payload


@pytest.mark.parametrize("case", IC.corrupt_cases(), ids=lambda c: c[0])
def test_corrupt_member_then_a_good_file(product, case):
    _, m = case
    rc, _, bad, msg = product.bgzf_inflate(IC.corrupt_file(m), 0)
    assert (rc, bad, msg) == (G2S_ERR_IO, 1, "corrupt BGZF block 1")
    data, payload = IC.good_file_after()
    assert product.bgzf_inflate(data, 0)[:2] == (G2S_OK, payload)


def test_random_corpus(product):
    data, payload = IC.random_corpus()
    rc, got, _, msg = product.bgzf_inflate(data, 0)
    assert rc == G2S_OK, msg
    assert got == payload


# ---- the batched filter, end to end

@functools.lru_cache(maxsize=None)
def _library(block):
    refs, recs, _ = BW.simulate_library(41, n_scaffolds=2, scaffold_len=12000, gap=(6000, 250), pairs=1500, unmapped_pairs=40)
    rng = random.Random(42)
    gaps = [(rng.choice(refs)[0], rng.randrange(500, 11500), rng.choice([-1, 0, rng.randrange(1, 400)]),
             rng.choice([-1, 0, rng.randrange(1, 150)])) for _ in range(40)] + [("scaf0", 6000, 250, 60), ("nosuch", 10, 5, 5)]
    return BW.bam_bytes(refs, recs, block=block), gaps


def _both(product, bam, gaps):
    texts, stats, un = product.filter_reads_gaps(bam, 300, 20, gaps, device=0, unmapped=True)
    hook = product.last_filter_inflate()
    pool = product.filter_reads_gaps_pool(bam, 300, 20, gaps, device=0)
    hook_pool = product.last_filter_inflate()
    got = (texts, un, [pool.fasta(i) for i in range(len(gaps))], pool.unmapped_fasta(), pool.n_reads, pool.total)
    passes = (stats["file_passes"], pool.stats["file_passes"], stats["on_device"], pool.stats["on_device"])
    pool.free()
    return got, passes, hook, hook_pool


@pytest.mark.parametrize("block", [65280, 5000, 700])
@pytest.mark.parametrize("chunk", [None, "windows"], ids=["one_window", "six_windows"])
def test_filter_with_device_inflate_equals_host_inflate(product, monkeypatch, block, chunk):
    bam, gaps = _library(block)
    rc, raw, _, _ = product.bgzf_inflate(bam, -1)
    assert rc == G2S_OK and len(raw) > 300000
    if chunk:
        monkeypatch.setenv("G2S_BAM_CHUNK", str(len(raw) // 6))  # six windows or more: look-ahead, carried bytes
    else:
        monkeypatch.delenv("G2S_BAM_CHUNK", raising=False)
    _device_inflate(monkeypatch, True)
    dev, dev_passes, dev_hook, dev_hook_pool = _both(product, bam, gaps)
    _device_inflate(monkeypatch, False)
    host, host_passes, host_hook, _ = _both(product, bam, gaps)
    assert dev_hook["on_device"] == 1 and dev_hook_pool["on_device"] == 1 and host_hook["on_device"] == 0
    assert dev_passes == host_passes == (2, 2, 1, 1)
    assert dev_hook["members"] == host_hook["members"] == 2 * len(IC.split_members(bam))
    assert dev_hook["bytes_out"] == host_hook["bytes_out"] == 2 * len(raw)
    assert dev == host
    assert sum(x[3] for x in dev[0]) > 100


def test_corrupt_member_in_the_second_window(product, monkeypatch):
    bam, gaps = _library(5000)
    members = IC.split_members(bam)
    bad = 6
    m = bytearray(members[bad])
    m[-5] ^= 0x10  # (a bit of its CRC-32)
    broken = b"".join(members[:bad]) + bytes(m) + b"".join(members[bad + 1:])
    monkeypatch.setenv("G2S_BAM_CHUNK", "20000")  # four members a window: member 6 is in the second
    seen = []
    for on in (True, False):
        _device_inflate(monkeypatch, on)
        for call in (product.filter_reads_gaps, product.filter_reads_gaps_pool):
            with pytest.raises(product.G2SError) as e:
                call(broken, 300, 20, gaps, device=0)
            seen.append((e.value.code, str(e.value.msg) if hasattr(e.value, "msg") else str(e.value)))
            hook = product.last_filter_inflate()
            assert hook["on_device"] == (1 if on else 0)  # (device: no window went to the host to "make sure")
    assert all(code == G2S_ERR_IO for code, _ in seen)
    assert all("corrupt BGZF block 6" in text for _, text in seen), seen


# ---- Gap2Seq-libraries

def test_libraries_output_does_not_depend_on_where_the_file_is_inflated(tmp_path):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    K, FUZ, length = 31, 10, 6000
    rng = random.Random(23)
    genome = "".join(rng.choice("ACGT") for _ in range(length))  # (simulate_library's first draws)
    lines = []
    for i, (pairs, mean, sd, thr) in enumerate([(900, 300, 20, 0.0), (400, 250, 30, 0.5), (600, 350, 0, 1000.0)]):
        refs, recs, _ = BW.simulate_library(23, n_scaffolds=1, scaffold_len=length, gap=(3000, 200), pairs=pairs, mean=mean,
                                            sd=sd, unmapped_pairs=10, ambiguous=0.0)
        (tmp_path / ("lib%d.bam" % i)).write_bytes(BW.bam_bytes(refs, recs, block=[65280, 5000, 700][i]))
        lines.append("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), mean, sd, thr))
    fl = K + FUZ
    records, bed = [], []
    for j, (bp, gl) in enumerate([(3000, 200), (700, 100), (2200, 150), (4600, 80), (5200, 120), (1600, 90)]):
        records.append(">scaf0 scaffold 0 contig %d gap %d\n%s\n" % (j, j, genome[bp - fl:bp] + "N" * gl + genome[bp + gl:bp + gl + fl]))
        bed.append("scaf0\t%d\t%d\n" % (bp - fl, bp + gl + fl))
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join(lines))
    outs = []
    for name, env in (("dev", {"G2S_DEVICE_INFLATE": "1"}), ("host", {"G2S_HOST_INFLATE": "1"})):
        e = {k: v for k, v in os.environ.items() if k not in ("G2S_HOST_INFLATE", "G2S_DEVICE_INFLATE", "G2S_HOST_FILTER")}
        e.update(env)
        out = tmp_path / (name + ".fa")
        run = subprocess.run([EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                              str(tmp_path / "gaps.bed"), "-filled", str(out), "-k", str(K), "-fuz", str(FUZ), "-solid", "1",
                              "-dist-error", "100", "-randseed", "3"], capture_output=True, text=True, timeout=300, env=e)
        assert run.returncode == 0, run.stderr
        outs.append((out.read_bytes(), run.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert b">" in outs[0][0]
