"""The kernels of gap2seq_amd/csrc/gzip_inflate.hip (k_gz_find, k_gz_decode, k_gz_chain, k_gz_resolve, k_gz_crc) on the
designed files of gzip_cases.py: through the hook against Python's zlib and against the same algorithm compiled for the
host (their outcomes and counts must be the same, not only the bytes), and through the loader — reads_text,
Graph.from_files, Gap2Seq-core — where a file the route gives back is read by zlib and nothing else may change.
tests/test_gzip_chunks.py says which outcome each case expects and why."""
import json
import os
import subprocess

import pytest

import fastx_model as M
import gzip_cases as G
from test_gzip_chunks import CHUNKS, LEVELS, WINDOWS, check_design_stats, inflate_checked, must_complete
from test_reads_text import _assert_same_graph

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCHES = ("G2S_HOST_BUILD", "G2S_HOST_READS", "G2S_HOST_INFLATE", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES",
            "G2S_BUILD_TEXT_FIRST_BYTES", "G2S_DEVICE_GZIP", "G2S_GZIP_CHUNK_BYTES", "G2S_GZIP_WINDOW_CHUNKS", "G2S_GZIP_SLOT_RATIO")
COUNTS = ("windows", "chunks", "starts_found", "absorbed", "members", "outcome")


@pytest.fixture(autouse=True)
def no_switches(product, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    yield
    product.set_device_gzip(-1)


def same_as_host(product, data, chunk, window, dev_outcome, dev_stats):
    got, outcome = product.gzip_inflate(data, -2, chunk, window)
    host = product.last_reads_gzip()
    assert outcome == dev_outcome and [host[c] for c in COUNTS] == [dev_stats[c] for c in COUNTS]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("level", LEVELS)
def test_fastq_text(product, level, chunk, window):
    data, payload = G.fastq_gz(level), G.fastq_text()
    outcome, st = inflate_checked(product, data, payload, 0, chunk, window, must_complete(chunk, window))
    same_as_host(product, data, chunk, window, outcome, st)
    assert st["peak_device_bytes"] > 0
    if outcome == "done" and chunk == 65536:
        assert st["absorbed"] <= 2
    if outcome == "done" and chunk == 4096:
        assert st["absorbed"] > st["chunks"] // 2


@pytest.mark.parametrize("chunk,window", [(4096, 0), (4096, 17), (16384, 0), (65536, 0)])
def test_history_across_chunks(product, chunk, window):
    data, payload, starts, notes = G.history_design()
    outcome, st = inflate_checked(product, data, payload, 0, chunk, window, True)
    if window == 0:
        check_design_stats(st, starts, chunk, len(data))


@pytest.mark.parametrize("window", [0, 3])
def test_markers_of_markers(product, window):
    data, payload, starts = G.relay_design()
    outcome, st = inflate_checked(product, data, payload, 0, 16384, window, True)
    if window == 0:
        check_design_stats(st, starts, 16384, len(data))


@pytest.mark.parametrize("name,data,payload,members", G.member_cases(), ids=[c[0] for c in G.member_cases()])
@pytest.mark.parametrize("window", [0, 4])
def test_members(product, name, data, payload, members, window):
    outcome, st = inflate_checked(product, data, payload, 0, 4096, window, True)
    assert st["members"] == members


def reads_text_with_the_mode(product, data, monkeypatch, chunk=4096, piece=10000):
    """(the device loader's text with the mode asked for, the host loader's, what the loader says, what the route says)"""
    monkeypatch.setenv("G2S_GZIP_CHUNK_BYTES", str(chunk))
    want = product.reads_text(data, device=-1)
    product.set_device_gzip(1)
    got = product.reads_text(data, device=0, piece_bytes=piece)
    return got, want, product.last_reads_load(), product.last_reads_gzip()


@pytest.mark.parametrize("name,data,payload", G.startless_cases(), ids=[c[0] for c in G.startless_cases()])
def test_no_usable_start(product, monkeypatch, name, data, payload):
    assert product.gzip_inflate(data, 0, 4096, 2) == (b"", "too few starts")
    assert product.gzip_inflate(data, 0, 4096, 0) == (payload, "done")
    if name == "one-dynamic-block":  # (no read file: the hook's bytes are the whole of it)
        return
    got, want, load, route = reads_text_with_the_mode(product, data, monkeypatch)
    assert got == want and len(want) > 50000
    assert (load["inflate"], load["on_device"], route["files"], route["outcome"]) == (["zlib"], 1, 1, "too few starts")
    assert load["raw_bytes"] == len(payload)


@pytest.mark.parametrize("name,data,payload", G.flushed_cases(), ids=[c[0] for c in G.flushed_cases()])
def test_flushed_streams_decode_on_the_device(product, monkeypatch, name, data, payload):
    outcome, st = inflate_checked(product, data, payload, 0, 4096, 4, True)
    same_as_host(product, data, 4096, 4, outcome, st)
    monkeypatch.setenv("G2S_GZIP_WINDOW_CHUNKS", "5")
    got, want, load, route = reads_text_with_the_mode(product, data, monkeypatch)
    assert got == want and len(want) > 100000
    assert (load["inflate"], load["on_device"], route["outcome"], route["members"]) == (["device-gzip"], 1, "done", 1)
    assert load["raw_bytes"] == len(payload) and route["windows"] * 5 >= route["chunks"] >= 15 and route["peak_device_bytes"] > 0


def test_a_false_start_is_a_boundary_mismatch(product, monkeypatch):
    """a handled input: the chunk in front of the false start ends in a status word, and zlib reads the file"""
    data, payload, false_bit = G.false_start_design()
    assert product.gzip_inflate(data, 0, 4096, 0) == (b"", "boundary mismatch")
    assert product.gzip_inflate(data, 0, 65536, 0) == (payload, "done")
    got, want, load, route = reads_text_with_the_mode(product, data, monkeypatch)
    assert got == want and got.count(b"N") == 3
    assert (load["inflate"], route["outcome"]) == (["zlib"], "boundary mismatch")


def test_a_full_slot_rewinds_behind_another_file(product, monkeypatch, tmp_path):
    data, payload = G.repeated_line()
    monkeypatch.setenv("G2S_GZIP_SLOT_RATIO", "8")
    assert product.gzip_inflate(data, 0, 4096, 0) == (b"", "slot full")
    got, want, load, route = reads_text_with_the_mode(product, data, monkeypatch)
    assert got == want and (load["inflate"], route["outcome"]) == (["zlib"], "slot full")
    # a FASTA file in front of it: the rewind goes back to where the second file's text began
    genome, reads = M.base_reads()
    same = M.records(payload)[0].decode()
    a, b = tmp_path / "a.fa", tmp_path / "b.fq.gz"
    a.write_bytes(M.fasta(reads))
    b.write_bytes(data)
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "10000")
    ref = product.Graph.from_seqs(reads + [same] * payload.count(b"@same"), 31, 2)
    g = product.Graph.from_files("%s,%s" % (a, b), 31, 2)
    try:
        load, route = product.last_reads_load(), product.last_reads_gzip()
        assert (load["on_device"], load["inflate"], route["outcome"]) == (1, ["none", "zlib"], "slot full")
        assert load["records"] == len(reads) + payload.count(b"@same")
        x, y = product.test_graph_tables(g), product.test_graph_tables(ref)
        assert g.num_kmers == ref.num_kmers and bytes(x[0]) == bytes(y[0]) and bytes(x[1]) == bytes(y[1])
    finally:
        g.free()
        ref.free()


@pytest.mark.parametrize("how", ["truncated", "flipped-deflate-byte", "flipped-crc-byte"])
def test_damage_has_zlibs_message(product, monkeypatch, how):
    data = G.damaged(G.small_blocks_gz(G.fastq_text()[:150000]), how)
    got, outcome = product.gzip_inflate(data, 0, 4096, 0)
    assert got == b"" and outcome in ("corrupt", "trailer", "boundary mismatch")
    monkeypatch.setenv("G2S_GZIP_CHUNK_BYTES", "4096")
    with pytest.raises(product.G2SError) as off:
        product.reads_text(data, device=0, piece_bytes=10000)
    product.set_device_gzip(1)
    with pytest.raises(product.G2SError) as on:
        product.reads_text(data, device=0, piece_bytes=10000)
    assert str(on.value) == str(off.value)


@pytest.fixture(scope="module")
def ref_graph(product):
    genome, reads = M.base_reads()
    g = product.Graph.from_seqs(reads, 31, 2)
    yield genome, reads, g
    g.free()


@pytest.mark.parametrize("way", ["call", "environment", "unset"])
def test_from_files_by_each_way_of_asking(product, ref_graph, monkeypatch, tmp_path, way):
    genome, reads, ref = ref_graph
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(G.small_blocks_gz(M.fastq(reads)))
    monkeypatch.setenv("G2S_GZIP_CHUNK_BYTES", "4096")
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "10000")
    if way == "call":
        product.set_device_gzip(1)
    elif way == "environment":
        monkeypatch.setenv("G2S_DEVICE_GZIP", "1")
    g = product.Graph.from_files(str(path), 31, 2)
    try:
        load, route = product.last_reads_load(), product.last_reads_gzip()
        print(way, load, route)
        if way == "unset":
            assert (load["inflate"], load["on_device"], route["files"]) == (["zlib"], 1, 0)
        else:
            assert (load["inflate"], load["on_device"], route["outcome"], route["members"]) == (["device-gzip"], 1, "done", 1)
            assert route["starts_found"] * 4 >= route["chunks"] >= 12
        assert load["records"] == len(reads) and load["positions"] == sum(len(r) + 1 for r in reads)
        a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
        assert g.num_kmers == ref.num_kmers and bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
        _assert_same_graph(g, ref, 31, [genome], 33)
    finally:
        g.free()


def test_command_line_asks_for_it(product, tmp_path):
    """Gap2Seq-core -device-gzip 1 on tests/golden/scaffold_cases.json's reads writes what it writes from plain FASTA"""
    sc = json.load(open(os.path.join(HERE, "golden", "scaffold_cases.json")))
    scaf = tmp_path / "scaf.fa"
    scaf.write_text(sc["scaffolds"])
    fq = M.fastq(sc["seqs"])
    outs, logs = {}, {}
    env = dict(os.environ, G2S_GZIP_CHUNK_BYTES="1024", G2S_DEBUG="1")
    env.pop("G2S_DEVICE_GZIP", None)
    for name, data, more in (("reads.fa", M.fasta(sc["seqs"]), []), ("reads.fq.gz", G.gz(fq, mem_level=1), ["-device-gzip", "1"]),
                             ("off.fq.gz", G.gz(fq, mem_level=1), ["-device-gzip", "0"])):
        (tmp_path / name).write_bytes(data)
        out = tmp_path / (name + ".filled.fa")
        res = subprocess.run([os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-core"), "-k", str(sc["k"]), "-fuz", str(sc["max_fuz"]),
                              "-solid", str(sc["solid"]), "-nb-cores", "1", "-dist-error", str(sc["d_err"]), "-max-mem", "20",
                              "-randseed", str(sc["randseed"]), "-reads", str(tmp_path / name), "-filled", str(out),
                              "-scaffolds", str(scaf)] + more, capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        outs[name], logs[name] = out.read_bytes(), res.stderr
    assert len(outs["reads.fa"]) > 0 and b">" in outs["reads.fa"]
    assert outs["reads.fq.gz"] == outs["reads.fa"] and outs["off.fq.gz"] == outs["reads.fa"]
    assert "reads.fq.gz: inflated on the device, 1 members" in logs["reads.fq.gz"]
    assert "inflated on the device" not in logs["off.fq.gz"]
