"""The streaming form of the BAM read route (gap2seq_amd/csrc/bam_reads.h): the file through the inflate's two slots
window by window, every walk window's records turned into text by k_bamstream_len / k_bamstream_write right behind its
row kernels, device memory bounded by the text and a fixed amount.  The text must be the host route's byte for byte, the
graph Graph.from_seqs' word for word, and g2s_test_last_reads_bam_stream keeps a case from passing through another
route.  Cases: tests/bam_reads_cases.py; the windows' model and the file over the cap: tests/bam_stream_cases.py."""
import pytest

import bam_reads_cases as B
import bam_stream_cases as S
import bamwriter
import fastx_model as M
from test_gpu_bam_reads import CASES, CASE_PIECES, ROWS_CARRY, SWITCHES, _same_tables, _valid_keys
from test_reads_text import _assert_same_graph

pytestmark = pytest.mark.gpu

STREAM = "G2S_BUILD_BAM_STREAM"
PIECE, BLOCK = 10000, 3000  # test 3: the window, and the members it is made of
ROWS_CORRUPT = 7  # (csrc/bam_rows.h: kRowsCorrupt)
G2S_ERR_HIP = -4  # (include/g2s.h)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES + (STREAM,):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def host_texts(product):
    """the host route's text of every case, made once"""
    return {name: product.reads_text(data, device=-1) for name, data, _, _ in CASES}


def _assert_streamed_text(product, data, recs, piece, want):
    got = product.reads_text(data, device=0, piece_bytes=piece)
    info, bam, stream = product.last_reads_load(), product.last_reads_bam(), product.last_reads_bam_stream()
    print(info, bam, stream)
    assert got == want == B.text(recs)
    kept = len(B.reads(recs))
    assert bam == dict(files=1, kept=kept, skipped=len(recs) - kept, kernels=1, reason="kernels", anomaly=0)
    assert (info["on_device"], info["records"], info["positions"], info["inflate"]) == (1, kept, len(got), ["device"])
    assert (stream["streamed_files"], info["grows"]) == (1, 0)  # (the text buffer is sized from the stream's bytes, once)
    assert info["pieces"] == stream["windows"]
    if piece:
        inflated = B.first_record() + sum(len(r) for r in recs)
        assert stream["windows"] >= (inflated - B.first_record()) // piece
    return stream


# ---- 1: the text, byte for byte


@pytest.mark.parametrize("name,data,recs,piece", CASE_PIECES, ids=["%s-%d" % (c[0], c[3]) for c in CASE_PIECES])
def test_streamed_text_is_the_host_routes(product, host_texts, monkeypatch, name, data, recs, piece):
    monkeypatch.setenv(STREAM, "1")
    _assert_streamed_text(product, data, recs, piece, host_texts[name])


# ---- 2: a window's end in every field of a record

CUT_SEEDS = (1, 2, 3, 4)
CUT_WINDOWS = tuple(S.hold() + 100 * j for j in range(8))


def test_the_cut_cases_cut_every_field():
    """a condition on the inputs, checked without the device: over the files of the test below a window ends inside the
    fixed bytes, the name, the CIGAR, the packed bases and the qualities of some record"""
    hit = set()
    for seed in CUT_SEEDS:
        recs = B.length_records(seed)
        for piece in CUT_WINDOWS:
            hit |= S.cut_fields(recs, 100, piece)
    assert hit == set(S.FIELDS)


@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_records_cut_in_every_field(product, monkeypatch, seed):
    monkeypatch.setenv(STREAM, "1")
    recs = B.length_records(seed)
    data = bamwriter.bam_bytes(B.REFS, recs, block=100)
    want = product.reads_text(data, device=-1)
    for piece in CUT_WINDOWS:
        assert S.cut_fields(recs, 100, piece)  # (every one of these windows cuts records)
        _assert_streamed_text(product, data, recs, piece, want)


# ---- 3, 4: a file over the resident cap


@pytest.fixture(scope="module")
def big(product):
    """(genome, records, BAM bytes, S, Graph.from_seqs of the reads): 250-base reads whose inflated stream behind the
    header is ten times the streaming form's fixed footprint at the test's window"""
    genome, recs = S.big_reads(10 * S.fixed_bound(PIECE, BLOCK))
    data = bamwriter.bam_bytes(B.REFS, recs, block=BLOCK)
    ref = product.Graph.from_seqs(B.reads(recs), 31, 2)
    assert product.test_last_solid_count()["on_device"] == 1 and ref.num_kmers > 100000
    yield genome, recs, data, sum(len(r) for r in recs), ref
    ref.free()


def _from_big(product, big, tmp_path, streamed):
    genome, recs, data, stream_bytes, ref = big
    reads = B.reads(recs)
    path = tmp_path / "big.bam"
    path.write_bytes(data)
    g = product.Graph.from_files(str(path), 31, 2)
    try:
        load, bam, stream = product.last_reads_load(), product.last_reads_bam(), product.last_reads_bam_stream()
        print(load, bam, stream, stream_bytes)
        assert (load["on_device"], bam["kernels"], stream["streamed_files"]) == ((1, 1, 1) if streamed else (0, 0, 0))
        assert (load["records"], bam["kept"], bam["skipped"]) == (len(reads), len(reads), len(recs) - len(reads))
        assert load["positions"] == sum(len(r) + 1 for r in reads)
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 17)
        return load, bam, stream
    finally:
        g.free()


def test_over_the_resident_cap_streams_by_default(product, big, tmp_path, monkeypatch):
    stream_bytes = big[3]
    fixed = S.fixed_bound(PIECE, BLOCK)
    assert stream_bytes >= 10 * fixed and 2 * stream_bytes // 3 + fixed < stream_bytes
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", str(PIECE))
    monkeypatch.setenv("G2S_BUILD_RESIDENT_CAP", str(stream_bytes))
    load, bam, stream = _from_big(product, big, tmp_path, streamed=True)
    assert (bam["reason"], load["grows"], load["inflate"]) == ("kernels", 0, ["device"])
    assert stream["peak_device_bytes"] <= stream_bytes
    # (the documented bound of the fixed part, and the text sized from two thirds of the stream)
    assert stream["peak_device_bytes"] <= fixed + S.device_text_bytes(2 * stream_bytes // 3)
    assert stream["windows"] >= stream_bytes // PIECE


def test_neither_route_fits(product, big, tmp_path, monkeypatch):
    """a cap above the fixed footprint and below the text: the text outgrows what the cap leaves, the host loader reads"""
    stream_bytes = big[3]
    text = sum(len(r) + 1 for r in B.reads(big[1]))
    assert S.fixed_bound(PIECE, BLOCK) < stream_bytes // 4 < text
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", str(PIECE))
    monkeypatch.setenv("G2S_BUILD_RESIDENT_CAP", str(stream_bytes // 4))
    load, bam, stream = _from_big(product, big, tmp_path, streamed=False)
    assert (bam["reason"], bam["anomaly"], load["on_device"], load["inflate"]) == ("over the cap", 0, 0, ["zlib"])
    assert stream == dict(streamed_files=0, windows=0, peak_device_bytes=0)


def test_the_switch_says_never(product, big, tmp_path, monkeypatch):
    """G2S_BUILD_BAM_STREAM=0: the file over the cap goes to the host loader as before"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", str(PIECE))
    monkeypatch.setenv("G2S_BUILD_RESIDENT_CAP", str(big[3]))
    monkeypatch.setenv(STREAM, "0")
    load, bam, stream = _from_big(product, big, tmp_path, streamed=False)
    assert (bam["reason"], stream["streamed_files"]) == ("over the cap", 0)


# ---- 5, 6: whole graphs with streaming forced


@pytest.fixture(scope="module")
def ref31(product):
    genome, recs = B.graph_reads(31)
    g = product.Graph.from_seqs(B.reads(recs), 31, 2)
    assert product.test_last_solid_count()["on_device"] == 1 and g.num_kmers > 1000
    yield genome, recs, g
    g.free()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_mixed_list(product, ref31, tmp_path, monkeypatch, where):
    """the streamed file's text lands behind what the list gave so far, and a FASTA/FASTQ file behind it in the right
    place: the position the device carried through the windows is the one the next file starts from"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "4000")
    monkeypatch.setenv(STREAM, "1")
    genome, recs, ref = ref31
    third = len(recs) // 3
    parts = [recs[:third], recs[third:2 * third], recs[2 * third:]]
    bam_at = ("first", "middle", "last").index(where)
    files, reads, how = [], [], []
    plain = min(i for i in range(3) if i != bam_at)  # (of the two others the first is FASTA, the second .fq.gz)
    for i, part in enumerate(parts):
        mine = B.reads(part)
        reads += mine
        if i == bam_at:
            data, h = bamwriter.bam_bytes(B.REFS, part, block=2500), "device"
        elif i == plain:
            data, h = M.fasta(mine, 60), "none"
        else:
            data, h = M.gz(M.fastq(mine)), "zlib"
        path = tmp_path / ("part%d%s" % (i, ".bam" if i == bam_at else ".fa" if i == plain else ".fq.gz"))
        path.write_bytes(data)
        files.append(str(path))
        how.append(h)
    g = product.Graph.from_files(",".join(files), 31, 2)
    try:
        load, bam, stream = product.last_reads_load(), product.last_reads_bam(), product.last_reads_bam_stream()
        print(load, bam, stream)
        assert (load["on_device"], load["files"], load["inflate"]) == (1, 3, how)
        assert (load["records"], load["positions"]) == (len(reads), sum(len(r) + 1 for r in reads))
        kept = len(B.reads(parts[bam_at]))
        assert bam == dict(files=1, kept=kept, skipped=len(parts[bam_at]) - kept, kernels=1, reason="kernels", anomaly=0)
        assert stream["streamed_files"] == 1 and stream["windows"] >= sum(map(len, parts[bam_at])) // 4000
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 12)
    finally:
        g.free()


def test_key_range_passes_read_the_slack_as_padding(product, ref31, tmp_path, monkeypatch):
    """the text buffer is a tile and more larger than the text needs: the key-range passes still read 'N' behind the
    text's end"""
    genome, recs, ref = ref31
    reads = B.reads(recs)
    recs = [S.renamed(r, "read_%03d_" % i + "n" * 240) for i, r in enumerate(recs)]  # (a longer stream for the same text)
    assert B.reads(recs) == reads
    monkeypatch.setenv("G2S_BUILD_PASS_KEYS", str(_valid_keys(reads, 31) // 3))
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "1000")
    monkeypatch.setenv(STREAM, "1")
    path = tmp_path / "reads.bam"
    path.write_bytes(bamwriter.bam_bytes(B.REFS, recs, block=700))
    g = product.Graph.from_files(str(path), 31, 2)
    try:
        load, count, stream = product.last_reads_load(), product.test_last_solid_count(), product.last_reads_bam_stream()
        print(load, count, stream)
        text = sum(len(r) + 1 for r in reads)
        # (a condition on the input: the buffer sized from two thirds of the stream has whole tiles behind the text)
        assert S.device_text_bytes(2 * sum(map(len, recs)) // 3) >= S.device_text_bytes(text) + 16384
        assert (load["on_device"], stream["streamed_files"], count["on_device"]) == (1, 1, 1)
        assert load["positions"] == count["positions"] == text and count["passes"] >= 3
        assert stream["peak_device_bytes"] > S.device_text_bytes(text) + 2 * S.FRONT
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 14)
    finally:
        g.free()


# ---- 7: ways out


def test_a_record_longer_than_the_room_in_front_of_a_window(product, tmp_path, monkeypatch):
    """a record of 450 000 bytes cut by the ends of 64 KiB windows: its head does not fit the 256 KiB in front of one"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "65536")
    monkeypatch.setenv(STREAM, "1")
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
        load, bam, stream = product.last_reads_load(), product.last_reads_bam(), product.last_reads_bam_stream()
        print(load, bam, stream)
        assert (load["on_device"], load["inflate"], load["records"]) == (0, ["zlib"], len(reads))
        assert (bam["kernels"], bam["reason"], bam["anomaly"], bam["kept"]) == (0, "rows anomaly", ROWS_CARRY, len(reads))
        assert stream["streamed_files"] == 0
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, 31, [genome], 13)
    finally:
        g.free()
        ref.free()


def test_a_corrupt_member_in_a_later_window(product, tmp_path, monkeypatch):
    """a byte flipped inside the deflate bytes of a member of the fourth window: an error that names the file"""
    monkeypatch.setenv("G2S_BUILD_PIECE_BYTES", "4000")
    monkeypatch.setenv(STREAM, "1")
    # (the reader parses the header on the host in windows of its own, 32 MiB unless this says otherwise: with the
    # whole file in the first of them the damaged member would be met when the file is opened, before any route)
    monkeypatch.setenv("G2S_BAM_CHUNK", "4000")
    _, recs = B.graph_reads(31)
    whole = bamwriter.bam_bytes(B.REFS, recs, block=2000)
    members, o = [], 0
    while o < len(whole):  # (a member's size - 1 is the value of its BC subfield)
        members.append(o)
        o += int.from_bytes(whole[o + 16:o + 18], "little") + 1
    assert o == len(whole) and len(members) > 12
    at = members[7] + 18 + (members[8] - members[7] - 26) // 2  # (two members a window: the fourth window's second)
    data = bytearray(whole)
    data[at] ^= 0x55
    path = tmp_path / "damaged.bam"
    path.write_bytes(bytes(data))
    with pytest.raises(product.G2SError) as e:
        product.Graph.from_files(str(path), 31, 2).free()
    assert e.value.code == product.G2S_ERR_IO and "damaged.bam" in str(e.value)
    # (the hooks speak of the last call that built a graph, so after this error they cannot say which route met the
    # member.  The text hook never puts the host in the device's place: there the streaming form itself gives the
    # file back, as a member that did not inflate)
    with pytest.raises(product.G2SError) as e:
        product.reads_text(bytes(data), device=0, piece_bytes=4000)
    assert e.value.code == G2S_ERR_HIP
    bam = product.last_reads_bam()
    assert (bam["files"], bam["kernels"], bam["reason"], bam["anomaly"]) == (1, 0, "rows anomaly", ROWS_CORRUPT)
    assert product.last_reads_bam_stream()["streamed_files"] == 0
