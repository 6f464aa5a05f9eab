"""BAM files as read files of the graph build, on the device (gap2seq_amd/csrc/bam_reads.hip): the file inflated into
one device allocation with its rows beside it, the text made by k_bamreads_len / k_bamreads_write in windows that cut
records anywhere.  The text must be the host route's byte for byte, the graph Graph.from_seqs' word for word, and
g2s_test_last_reads_bam / g2s_test_last_reads_load keep a case from passing through a fallback.  Cases and model:
tests/bam_reads_cases.py."""
import json
import os
import subprocess

import pytest

import bam_reads_cases as B
import bamwriter
import fastx_model as M
from test_reads_text import _assert_same_graph

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCHES = ("G2S_HOST_BUILD", "G2S_HOST_READS", "G2S_HOST_INFLATE", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES",
            "G2S_BUILD_TEXT_FIRST_BYTES", "G2S_BUILD_RESIDENT_CAP", "G2S_BAM_CHUNK")
CASES = B.cases()
CASE_PIECES = [(name, data, recs, p) for name, data, recs, pieces in CASES for p in pieces]
ROWS_CARRY = 3  # (csrc/bam_rows.h: kRowsCarry)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def host_texts(product):
    """the host route's text of every case, made once"""
    return {name: product.reads_text(data, device=-1) for name, data, _, _ in CASES}


@pytest.mark.parametrize("name,data,recs,piece", CASE_PIECES, ids=["%s-%d" % (c[0], c[3]) for c in CASE_PIECES])
def test_device_text_is_the_host_routes(product, host_texts, name, data, recs, piece):
    got = product.reads_text(data, device=0, piece_bytes=piece)
    info, bam = product.last_reads_load(), product.last_reads_bam()
    assert got == host_texts[name] == B.text(recs)
    kept = len(B.reads(recs))
    assert bam == dict(files=1, kept=kept, skipped=len(recs) - kept, kernels=1, reason="kernels", anomaly=0)
    assert (info["on_device"], info["records"], info["positions"], info["inflate"]) == (1, kept, len(got), ["device"])
    assert info["grows"] == 0  # (the text buffer is sized from the count)
    if piece:
        inflated = B.first_record() + sum(len(r) for r in recs)
        assert info["pieces"] >= (inflated - B.first_record()) // piece
        assert name == "library" or info["raw_bytes"] == inflated


def test_host_inflate_switch_sends_bam_to_zlib(product, host_texts, monkeypatch):
    monkeypatch.setenv("G2S_HOST_INFLATE", "1")
    name, data, recs, _ = [c for c in CASES if c[0] == "lengths-members-100"][0]
    assert product.reads_text(data, device=0, piece_bytes=1000) == host_texts[name]
    assert product.last_reads_load()["inflate"] == ["zlib"]
    bam = product.last_reads_bam()
    assert (bam["kernels"], bam["reason"], bam["kept"]) == (0, "not asked", len(B.reads(recs)))


# ---- whole graphs


def _same_tables(product, g, ref):
    a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
    assert g.num_kmers == ref.num_kmers and bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])


@pytest.fixture(scope="module")
def refs(product):
    """Graph.from_seqs of the model's reads on the device, a graph per k, built once"""
    assert not any(os.environ.get(s) for s in SWITCHES)
    cache = {}

    def get(k):
        if k not in cache:
            genome, recs = B.graph_reads(k)
            g = product.Graph.from_seqs(B.reads(recs), k, 2)
            assert product.test_last_solid_count()["on_device"] == 1 and g.num_kmers > 1000
            cache[k] = (genome, recs, g)
        return cache[k]
    yield get
    for _, _, g in cache.values():
        g.free()


def _from_bam(product, refs, tmp_path, k, passes=False, kernels=True, **bgzf_args):
    genome, recs, ref = refs(k)
    reads = B.reads(recs)
    path = tmp_path / "reads.bam"
    path.write_bytes(bamwriter.bam_bytes(B.REFS, recs, **bgzf_args))
    g = product.Graph.from_files(str(path), k, 2)
    try:
        load, count, bam = product.last_reads_load(), product.test_last_solid_count(), product.last_reads_bam()
        print(load, count, bam)
        assert (load["on_device"], bam["kernels"]) == ((1, 1) if kernels else (0, 0))
        assert count["on_device"] == 1
        assert load["inflate"] == ["device" if kernels else "zlib"]
        assert load["positions"] == count["positions"] == sum(len(r) + 1 for r in reads)
        assert (load["records"], bam["kept"], bam["skipped"]) == (len(reads), len(reads), len(recs) - len(reads))
        assert (count["passes"] >= 3) if passes else (count["passes"] == 0)
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, k, [genome], k + 2)
        return bam
    finally:
        g.free()


@pytest.mark.parametrize("k", [31, 64])
def test_from_files_on_the_device(product, refs, tmp_path, monkeypatch, k):
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "10000")
    assert _from_bam(product, refs, tmp_path, k, block=3000)["reason"] == "kernels"


def test_from_files_default_window(product, refs, tmp_path):
    assert _from_bam(product, refs, tmp_path, 31)["reason"] == "kernels"


def _valid_keys(reads, k):
    n = 0
    for r in reads:
        bad = -1
        for i, c in enumerate(r):
            if c in "Nn":
                bad = i
            if i >= k - 1 and i - bad >= k:
                n += 1
    return n


def test_from_files_in_key_range_passes(product, refs, tmp_path, monkeypatch):
    _, recs, _ = refs(31)
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", str(_valid_keys(B.reads(recs), 31) // 3))
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "1000")
    _from_bam(product, refs, tmp_path, 31, passes=True, block=700)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_mixed_list(product, refs, tmp_path, monkeypatch, where):
    """the BAM file's text lands behind what the list gave so far, and a FASTA/FASTQ file behind it in the right place"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "4000")
    genome, recs, ref = refs(31)
    third = len(recs) // 3
    parts = [recs[:third], recs[third:2 * third], recs[2 * third:]]
    bam_at = ("first", "middle", "last").index(where)
    files, reads, how = [], [], []
    for i, part in enumerate(parts):
        mine = B.reads(part)
        reads += mine
        if i == bam_at:
            data, h = bamwriter.bam_bytes(B.REFS, part, block=2500), "device"
        elif (i + bam_at) % 2:
            data, h = M.gz(M.fastq(mine)), "zlib"
        else:
            data, h = bamwriter.bgzf(M.fasta(mine, 60), block=4000), "device"
        path = tmp_path / ("part%d" % i)
        path.write_bytes(data)
        files.append(str(path))
        how.append(h)
    g = product.Graph.from_files(",".join(files), 31, 2)
    try:
        load, bam = product.last_reads_load(), product.last_reads_bam()
        print(load, bam)
        assert (load["on_device"], load["files"], load["inflate"]) == (1, 3, how)
        assert (load["records"], load["positions"]) == (len(reads), sum(len(r) + 1 for r in reads))
        kept = len(B.reads(parts[bam_at]))
        assert bam == dict(files=1, kept=kept, skipped=len(parts[bam_at]) - kept, kernels=1, reason="kernels", anomaly=0)
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 12)
    finally:
        g.free()


# ---- ways out


def test_over_the_cap_goes_to_the_host_loader(product, refs, tmp_path, monkeypatch):
    monkeypatch.setenv("G2S_BUILD_RESIDENT_CAP", "1")
    bam = _from_bam(product, refs, tmp_path, 31, kernels=False)
    assert (bam["reason"], bam["anomaly"]) == ("over the cap", 0)


def test_a_record_longer_than_the_room_in_front_of_a_window(product, tmp_path, monkeypatch):
    """a record of 450 000 bytes cut by the ends of 64 KiB windows: its head does not fit the 256 KiB in front of one"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "65536")
    genome, recs = B.graph_reads(31)
    long_read = (genome * 30)[:300000]
    recs = recs[:20] + [bamwriter.record("long", 16, 0, 7, "300000M", bamwriter.revcomp(long_read))] + recs[20:]
    reads = B.reads(recs)
    assert long_read in reads
    path = tmp_path / "long.bam"
    path.write_bytes(bamwriter.bam_bytes(B.REFS, recs))
    ref = product.Graph.from_seqs(reads, 31, 2)
    g = product.Graph.from_files(str(path), 31, 2)
    try:
        load, bam = product.last_reads_load(), product.last_reads_bam()
        print(load, bam)
        assert (load["on_device"], load["inflate"], load["records"]) == (0, ["zlib"], len(reads))
        assert (bam["kernels"], bam["reason"], bam["anomaly"], bam["kept"]) == (0, "rows anomaly", ROWS_CARRY, len(reads))
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 13)
    finally:
        g.free()
        ref.free()


def test_host_reads_switch(product, refs, tmp_path, monkeypatch):
    monkeypatch.setenv("G2S_HOST_READS", "1")
    bam = _from_bam(product, refs, tmp_path, 31, kernels=False)
    assert bam["reason"] == "not asked"


def test_command_line_reads_a_bam_file(product, tmp_path):
    """Gap2Seq-core on tests/golden/scaffold_cases.json's read set as plain FASTA and as BAM"""
    sc = json.load(open(os.path.join(HERE, "golden", "scaffold_cases.json")))
    scaf = tmp_path / "scaf.fa"
    scaf.write_text(sc["scaffolds"])
    recs = [bamwriter.record("r%d" % i, 4, -1, -1, "", s) for i, s in enumerate(sc["seqs"])]
    assert B.reads(recs) == [s.upper() for s in sc["seqs"]]
    outs = {}
    for name, data in (("reads.fa", M.fasta(sc["seqs"])), ("reads.bam", bamwriter.bam_bytes(B.REFS, recs, block=3000))):
        (tmp_path / name).write_bytes(data)
        out = tmp_path / (name + ".filled.fa")
        res = subprocess.run([os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-core"), "-k", str(sc["k"]), "-fuz", str(sc["max_fuz"]),
                              "-solid", str(sc["solid"]), "-nb-cores", "1", "-dist-error", str(sc["d_err"]), "-max-mem", "20",
                              "-randseed", str(sc["randseed"]), "-reads", str(tmp_path / name), "-filled", str(out),
                              "-scaffolds", str(scaf)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        outs[name] = out.read_bytes()
    assert len(outs["reads.fa"]) > 0 and b">" in outs["reads.fa"]
    assert outs["reads.bam"] == outs["reads.fa"]
