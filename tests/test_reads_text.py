"""Graphs straight from read files, the part that needs no device: the host loader reads plain, gzip and BGZF files
(recognised by their magic bytes), its text is parse_fastx's, and the kernels' state machine (csrc/fastx_machine.h),
walked on the host, gives the same text.  The model is tests/fastx_model.py, a restatement of fastx.cpp."""
import random

import pytest

import bamwriter
import fastx_model as M

INVALID = 0xFFFFFFFF
ALL_PLAIN = M.base_cases() + M.machine_cases() + [M.long_line_case(), M.many_heads_case()]


@pytest.mark.parametrize("name,data", ALL_PLAIN, ids=[c[0] for c in ALL_PLAIN])
def test_hook_host_text_is_the_models(product, name, data):
    want = M.text(data)
    assert product.reads_text(data, device=-1) == want
    info = product.last_reads_load()
    assert (info["files"], info["raw_bytes"], info["positions"], info["records"], info["on_device"]) == \
        (1, len(data), len(want), len(M.records(data)), 0)
    # the table the kernels run, walked line by line on the host
    assert product.reads_text(data, device=-2) == want
    assert product.last_reads_load()["records"] == len(M.records(data))


@pytest.mark.parametrize("name,data,plain", M.compressed_cases(), ids=[c[0] for c in M.compressed_cases()])
def test_hook_host_text_of_compressed_input(product, name, data, plain):
    assert data[:2] == b"\x1f\x8b"
    assert product.reads_text(data, device=-1) == M.text(plain)
    assert product.reads_text(data, device=-2) == M.text(plain)
    assert product.last_reads_load()["raw_bytes"] == len(plain)


def _assert_same_graph(g, ref, k, sample_from, seed):
    assert (g.num_kmers, g.num_unitigs) == (ref.num_kmers, ref.num_unitigs)
    assert g.validate() == (0, "") and ref.validate() == (0, "")
    rr = random.Random(seed)
    hits = 0
    for _ in range(300):
        s = rr.choice(sample_from)
        if len(s) < k:
            continue
        p = rr.randrange(0, len(s) - k + 1)
        km = s[p:p + k].upper()
        x, y = g.node(km), ref.node(km)
        assert (x == INVALID) == (y == INVALID)
        if x != INVALID:
            hits += 1
            assert g.node_string(x) == km and ref.node_string(y) == km
            assert [g.node_string(v) for v in g.successors(x)] == [ref.node_string(v) for v in ref.successors(y)]
            assert [g.node_string(v) for v in g.predecessors(x)] == [ref.node_string(v) for v in ref.predecessors(y)]
    assert hits > 100


@pytest.fixture(scope="module")
def host_ref(product):
    """Graph.from_seqs of the base read set on the host, built once"""
    import os
    old = os.environ.get("G2S_HOST_BUILD")
    os.environ["G2S_HOST_BUILD"] = "1"
    try:
        genome, reads = M.base_reads()
        g = product.Graph.from_seqs(reads, 31, 2)
    finally:
        if old is None:
            del os.environ["G2S_HOST_BUILD"]
        else:
            os.environ["G2S_HOST_BUILD"] = old
    yield genome, reads, g
    g.free()


@pytest.mark.parametrize("form", ["fastq", "gzip", "bgzf", "bgzf-small-blocks", "bgzf-then-gzip"])
def test_from_files_on_the_host(product, host_ref, monkeypatch, tmp_path, form):
    genome, reads, ref = host_ref
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    fq = M.fastq(reads)
    assert [r.decode() for r in M.records(fq)] == reads
    data = {"fastq": fq, "gzip": M.gz(fq, 2), "bgzf": bamwriter.bgzf(fq), "bgzf-small-blocks": bamwriter.bgzf(fq, block=100, eof=False),
            "bgzf-then-gzip": bamwriter.bgzf(fq[:5000], block=700, eof=False) + M.gz(fq[5000:])}[form]
    path = tmp_path / ("reads.fq" if form == "fastq" else "reads.fq.gz")
    path.write_bytes(data)
    g = product.Graph.from_files(str(path), 31, 2)
    try:
        info = product.last_reads_load()
        assert info["on_device"] == 0 and info["files"] == 1 and info["raw_bytes"] == len(fq)
        assert info["inflate"] == ["none" if form == "fastq" else "zlib"]
        assert info["positions"] == sum(len(r) + 1 for r in reads) == product.test_last_solid_count()["positions"]
        _assert_same_graph(g, ref, 31, [genome], 3)
    finally:
        g.free()


def test_from_files_comma_list_mixing_forms(product, host_ref, monkeypatch, tmp_path):
    """two files, the first a gzip FASTQ that ends inside a record, the second BGZF FASTA: the parser starts afresh"""
    genome, reads, ref = host_ref
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    half = len(reads) // 2
    first = M.fastq(reads[:half]) + b"@cut\n"  # a header without its sequence: an empty record
    second = b"+\nstray line, ignored\n" + M.fasta(reads[half:], 60)
    a, b = tmp_path / "a.fq.gz", tmp_path / "b.fa.bgz"
    a.write_bytes(M.gz(first))
    b.write_bytes(bamwriter.bgzf(second, block=4000))
    want = M.records(first) + M.records(second)
    assert [r.decode() for r in want] == reads[:half] + [""] + reads[half:]
    g = product.Graph.from_files("%s,%s" % (a, b), 31, 2)
    try:
        info = product.last_reads_load()
        assert (info["files"], info["records"], info["inflate"]) == (2, len(want), ["zlib", "zlib"])
        assert info["positions"] == sum(len(r) + 1 for r in want)
        _assert_same_graph(g, ref, 31, [genome], 4)
    finally:
        g.free()


@pytest.mark.parametrize("damage", ["truncated", "flipped-byte", "truncated-bgzf"])
def test_damaged_gzip_is_an_error_naming_the_file(product, host_ref, monkeypatch, tmp_path, damage):
    _, reads, _ = host_ref
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    fq = M.fastq(reads)
    if damage == "truncated":
        data = M.gz(fq, 2)[:-20]  # inside the last member
    elif damage == "truncated-bgzf":
        data = bamwriter.bgzf(fq, eof=False)[:-20]
    else:
        data = bytearray(M.gz(fq, 2))
        data[len(data) // 3] ^= 0x55  # in the first member's deflate bytes
        data = bytes(data)
    path = tmp_path / "damaged.fq.gz"
    path.write_bytes(data)
    with pytest.raises(product.G2SError) as e:
        product.Graph.from_files(str(path), 31, 2).free()
    assert "damaged.fq.gz" in str(e.value)
    with pytest.raises(product.G2SError):
        product.reads_text(data, device=-1)


def test_missing_file_is_an_error(product, monkeypatch, tmp_path):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    with pytest.raises(product.G2SError) as e:
        product.Graph.from_files(str(tmp_path / "nothing.fq"), 31, 2).free()
    assert "nothing.fq" in str(e.value)


def test_a_pipe_is_read_on_the_host(product, host_ref, monkeypatch, tmp_path):
    """a FIFO, as `-reads <(zcat reads.fq.gz)` hands one over, plain and gzip"""
    import os
    import threading
    genome, reads, ref = host_ref
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    for n, data in enumerate((M.fastq(reads), M.gz(M.fastq(reads)))):
        fifo = str(tmp_path / ("reads%d.fifo" % n))
        os.mkfifo(fifo)

        def feed():
            with open(fifo, "wb") as f:
                f.write(data)
        t = threading.Thread(target=feed)
        t.start()
        try:
            g = product.Graph.from_files(fifo, 31, 2)
        finally:
            t.join()
        try:
            assert product.last_reads_load()["records"] == len(reads)
            _assert_same_graph(g, ref, 31, [genome], 8)
        finally:
            g.free()
