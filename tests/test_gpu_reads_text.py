"""Graphs straight from read files, on the device (gap2seq_amd/csrc/reads_text.hip): the build's text made by the
k_fastx_* kernels from the raw bytes of FASTA/FASTQ files, plain, gzip (zlib into the staging buffers) and BGZF (members
inflated on the device), in pieces that cut the file anywhere.  The text must be the host loader's byte for byte, the
graph Graph.from_seqs' word for word, and g2s_test_last_reads_load / g2s_test_last_solid_count keep a case from passing
through a fallback.  Cases and model: tests/fastx_model.py."""
import json
import os
import subprocess

import pytest

import bamwriter
import fastx_model as M
from test_reads_text import _assert_same_graph

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCHES = ("G2S_HOST_BUILD", "G2S_HOST_READS", "G2S_HOST_INFLATE", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES",
            "G2S_BUILD_TEXT_FIRST_BYTES")

PLAIN = M.base_cases() + M.machine_cases() + [M.long_line_case(), M.many_heads_case()]
PLAIN_PIECES = [(name, data, p) for name, data in PLAIN for p in M.piece_sizes(data)]
COMPRESSED_PIECES = [(name, data, plain, p) for name, data, plain in M.compressed_cases() for p in (16, 100, 1000, 1 << 20)]


@pytest.fixture(scope="module")
def host_texts(product):
    """the host loader's text of every case, made once"""
    texts = {name: product.reads_text(data, device=-1) for name, data in PLAIN}
    texts.update({name: product.reads_text(data, device=-1) for name, data, _ in M.compressed_cases()})
    return texts


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("name,data,piece", PLAIN_PIECES, ids=["%s-%d" % (c[0], c[2]) for c in PLAIN_PIECES])
def test_device_text_is_the_host_loaders(product, host_texts, name, data, piece):
    got = product.reads_text(data, device=0, piece_bytes=piece)
    info = product.last_reads_load()
    assert got == host_texts[name]
    assert (info["on_device"], info["positions"], info["raw_bytes"], info["inflate"]) == (1, len(got), len(data), ["none"])
    assert info["records"] == len(M.records(data)) and info["grows"] == 0
    assert info["pieces"] >= len(data) // piece


@pytest.mark.parametrize("name,data,plain,piece", COMPRESSED_PIECES, ids=["%s-%d" % (c[0], c[3]) for c in COMPRESSED_PIECES])
def test_device_text_of_compressed_input(product, host_texts, name, data, plain, piece):
    got = product.reads_text(data, device=0, piece_bytes=piece)
    info = product.last_reads_load()
    assert got == host_texts[name]
    want = "zlib" if name.startswith("gzip") else "mixed" if name == "bgzf-then-gzip" else "device"
    assert (info["on_device"], info["raw_bytes"], info["inflate"]) == (1, len(plain), [want])


def test_one_piece_of_many_tiles(product):
    """every thread of the one-workgroup scans walks several tiles"""
    name, data = M.one_piece_case()
    assert len(data) > 256 * 4096 * 4
    want = product.reads_text(data, device=-1)
    assert want == M.text(data)
    for piece in (len(data) + 4096, 3 << 20):
        got = product.reads_text(data, device=0, piece_bytes=piece)
        info = product.last_reads_load()
        assert got == want and (info["on_device"], info["records"]) == (1, len(M.records(data)))
        assert info["pieces"] == (1 if piece > len(data) else 2)


@pytest.mark.parametrize("name,data,plain,piece", M.bgzf_boundary_cases(), ids=[c[0] for c in M.bgzf_boundary_cases()])
def test_bgzf_windows_end_on_named_bytes(product, name, data, plain, piece):
    """a window is whole members up to a piece: with members of `piece` bytes the byte the device holds back is the named one"""
    got = product.reads_text(data, device=0, piece_bytes=piece)
    info = product.last_reads_load()
    assert got == M.text(plain)
    assert (info["on_device"], info["inflate"], info["raw_bytes"]) == (1, ["device"], len(plain))
    assert info["pieces"] >= len(plain) // piece  # (one member a window)


def test_a_pipe_goes_to_the_host_loader(product, refs, tmp_path):
    """a FIFO (as a process substitution is) is no file the device loader can size or map: the host loader reads it, once"""
    import threading
    genome, reads, ref = refs(31, 2)
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    data = M.gz(M.fastq(reads))

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
        load = product.last_reads_load()
        assert (load["on_device"], load["inflate"], load["records"]) == (0, ["zlib"], len(reads))
        assert g.num_kmers == ref.num_kmers
        _assert_same_graph(g, ref, 31, [genome], 9)
    finally:
        g.free()


def test_host_inflate_switch_sends_bgzf_to_zlib(product, host_texts, monkeypatch):
    monkeypatch.setenv("G2S_HOST_INFLATE", "1")
    name, data, plain = [c for c in M.compressed_cases() if c[0] == "bgzf-100-eof"][0]
    assert product.reads_text(data, device=0, piece_bytes=1000) == host_texts[name]
    assert product.last_reads_load()["inflate"] == ["zlib"]


def test_text_buffer_grows(product, host_texts, monkeypatch):
    monkeypatch.setenv("G2S_BUILD_TEXT_FIRST_BYTES", "64")
    name, data, plain = M.compressed_cases()[0]
    assert name == "gzip"
    assert product.reads_text(data, device=0, piece_bytes=1000) == host_texts[name]
    info = product.last_reads_load()
    print(info)
    assert info["grows"] >= 2 and info["on_device"] == 1


# ---- whole graphs


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


@pytest.fixture(scope="module")
def refs(product):
    """Graph.from_seqs of the base read set on the device (one sort), a graph per (k, solid), built once"""
    assert not any(os.environ.get(s) for s in SWITCHES)
    cache = {}

    def get(k, solid):
        if (k, solid) not in cache:
            genome, reads = M.base_reads(k)
            g = product.Graph.from_seqs(reads, k, solid)
            info = product.test_last_solid_count()
            assert (info["on_device"], info["passes"]) == (1, 0)
            cache[(k, solid)] = (genome, reads, g)
        return cache[(k, solid)]
    yield get
    for _, _, g in cache.values():
        g.free()


def _files(tmp_path, reads, form):
    fq = M.fastq(reads)
    half = len(reads) // 2
    if form == "two-files":
        a, b = tmp_path / "a.fq.gz", tmp_path / "b.fa.bgz"
        a.write_bytes(M.gz(M.fastq(reads[:half])))
        b.write_bytes(bamwriter.bgzf(M.fasta(reads[half:], 60), block=4000))
        return "%s,%s" % (a, b), ["zlib", "device"]
    data, how = {"fasta": (M.fasta(reads), "none"), "fastq": (fq, "none"), "fastq-crlf": (M.fastq(reads, "\r\n"), "none"),
                 "gzip": (M.gz(fq, 2), "zlib"), "bgzf": (bamwriter.bgzf(fq), "device"),
                 "bgzf-small-blocks": (bamwriter.bgzf(fq, block=100, eof=False), "device")}[form]
    path = tmp_path / ("reads." + form)
    path.write_bytes(data)
    return str(path), [how]


def _from_files_case(product, refs, tmp_path, form, k, solid, passes=False):
    genome, reads, ref = refs(k, solid)
    csv, how = _files(tmp_path, reads, form)
    g = product.Graph.from_files(csv, k, solid)
    try:
        load, count = product.last_reads_load(), product.test_last_solid_count()
        print(form, load, count)
        assert (load["on_device"], count["on_device"], load["inflate"]) == (1, 1, how)
        assert load["positions"] == count["positions"] == sum(len(r) + 1 for r in reads)
        assert load["records"] == len(reads) and count["solid"] == g.num_kmers
        assert (count["passes"] >= 3) if passes else (count["passes"] == 0)
        assert g.num_kmers == ref.num_kmers
        a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
        assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
        _assert_same_graph(g, ref, k, [genome], k + solid)
    finally:
        g.free()


@pytest.mark.parametrize("form", ["fasta", "fastq", "fastq-crlf", "gzip", "bgzf", "bgzf-small-blocks", "two-files"])
def test_from_files_on_the_device(product, refs, tmp_path, monkeypatch, form):
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "10000")  # (the files are cut into pieces)
    _from_files_case(product, refs, tmp_path, form, 31, 2)


def test_from_files_default_piece(product, refs, tmp_path):
    _from_files_case(product, refs, tmp_path, "fastq", 31, 2)


@pytest.mark.parametrize("k", [31, 64])
@pytest.mark.parametrize("form", ["fastq", "bgzf"])
def test_from_files_in_key_range_passes(product, refs, tmp_path, monkeypatch, form, k):
    _, reads, _ = refs(k, 2)
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", str(_valid_keys(reads, k) // 3))
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "1000")
    _from_files_case(product, refs, tmp_path, form, k, 2, passes=True)


def test_from_files_with_a_growing_text_buffer(product, refs, tmp_path, monkeypatch):
    monkeypatch.setenv("G2S_BUILD_TEXT_FIRST_BYTES", "64")
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "10000")
    _from_files_case(product, refs, tmp_path, "gzip", 31, 2)
    assert product.last_reads_load()["grows"] >= 2


def test_first_file_ends_inside_a_record(product, tmp_path, monkeypatch):
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "16")
    first, second = M.two_file_case()
    a, b = tmp_path / "a.fq", tmp_path / "b.fx"
    a.write_bytes(first)
    b.write_bytes(second)
    want = [r.decode() for r in M.records(first) + M.records(second)]
    ref = product.Graph.from_seqs(want, 3, 1)
    g = product.Graph.from_files("%s,%s" % (a, b), 3, 1)
    try:
        load = product.last_reads_load()
        assert (load["on_device"], load["files"], load["records"]) == (1, 2, len(want))
        assert load["positions"] == sum(len(r) + 1 for r in want)
        a_, b_ = product.test_graph_tables(g), product.test_graph_tables(ref)
        assert g.num_kmers == ref.num_kmers and bytes(a_[0]) == bytes(b_[0]) and bytes(a_[1]) == bytes(b_[1])
    finally:
        g.free()
        ref.free()


@pytest.mark.parametrize("form", ["fastq", "bgzf"])
def test_host_reads_switch(product, refs, tmp_path, monkeypatch, form):
    genome, reads, ref = refs(31, 2)
    monkeypatch.setenv("G2S_HOST_READS", "1")
    csv, _ = _files(tmp_path, reads, form)
    g = product.Graph.from_files(csv, 31, 2)
    try:
        load, count = product.last_reads_load(), product.test_last_solid_count()
        assert (load["on_device"], count["on_device"]) == (0, 1)  # (the host loader, then the device count as before)
        assert load["inflate"] == ["none" if form == "fastq" else "zlib"]
        a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
        assert g.num_kmers == ref.num_kmers and bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
    finally:
        g.free()


def test_command_line_reads_compressed_files(product, tmp_path):
    """Gap2Seq-core on tests/golden/scaffold_cases.json's read set as plain FASTA, as .fq.gz and as BGZF FASTQ"""
    sc = json.load(open(os.path.join(HERE, "golden", "scaffold_cases.json")))
    scaf = tmp_path / "scaf.fa"
    scaf.write_text(sc["scaffolds"])
    fq = M.fastq(sc["seqs"])
    outs = {}
    for name, data in (("reads.fa", M.fasta(sc["seqs"])), ("reads.fq.gz", M.gz(fq)), ("reads.bgzf.fq.gz", bamwriter.bgzf(fq, block=300))):
        (tmp_path / name).write_bytes(data)
        out = tmp_path / (name + ".filled.fa")
        res = subprocess.run([os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-core"), "-k", str(sc["k"]), "-fuz", str(sc["max_fuz"]),
                              "-solid", str(sc["solid"]), "-nb-cores", "1", "-dist-error", str(sc["d_err"]), "-max-mem", "20",
                              "-randseed", str(sc["randseed"]), "-reads", str(tmp_path / name), "-filled", str(out),
                              "-scaffolds", str(scaf)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        outs[name] = out.read_bytes()
    assert len(outs["reads.fa"]) > 0 and b">" in outs["reads.fa"]
    assert outs["reads.fq.gz"] == outs["reads.fa"] and outs["reads.bgzf.fq.gz"] == outs["reads.fa"]
