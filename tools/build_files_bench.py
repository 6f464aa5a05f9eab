#!/usr/bin/env python3
"""Time g2s_graph_build_files (Graph.from_files, Gap2Seq-core -reads) on bench.py's read sets written as FASTA, FASTQ,
gzip FASTQ and BGZF FASTQ: the device loader (gap2seq_amd/csrc/reads_text.hip, the default), the host loader
(G2S_HOST_READS=1), BGZF through zlib (G2S_HOST_INFLATE=1), and — on the two uncompressed files, all it can read —
another build of the library (--parent path/to/libg2s_hip.so, the commit before).  Every build runs in a process of its
own, so that its peak resident set is its own: the wall time is that of the one call, up to its return, behind a small
warm-up build that loads the runtime and the kernels; the resident set is the peak over the process less what the warm-up
left.  The ways alternate, --reps builds each; the median and the spread of each are printed as one JSON line.
--bam: the same reads as unaligned BAM records (a writer of this tool's own; --read-length L cuts bench.py's genome-long sequences into short reads of the same k-mers,
in every form) through the device route
(gap2seq_amd/csrc/bam_reads.hip) and through the host loader, beside --parent's library on the BGZF FASTQ file — what a
BAM file had to be converted to before BAM was read — and through the streaming form of the device route
(G2S_BUILD_BAM_STREAM=1: "stream bam"); --parent-bam has --parent's library read the BAM file too, both of its ways.

  python tools/build_files_bench.py --config C4 --reps 5 --threads 16 [--parent PATH/TO/libg2s_hip.so]
  python tools/build_files_bench.py --config C4 --once fastq     # one device-loader build in this process (kernel trace)
  python tools/build_files_bench.py --config C4 --bam --reps 5 [--parent PATH/TO/libg2s_hip.so [--parent-bam]]
  python tools/build_files_bench.py --config C4 --bam --read-length 250 --once bam     (or --once stream)
  python tools/build_files_bench.py --config C4 --gzip --reps 3 --parent PATH/TO/libg2s_hip.so [--genome BP] [--read-length L] [--slot-ratio R]
  python tools/build_files_bench.py --config C4 --gzip --once gzip [--chunk BYTES]    # the chunked device inflate, one build (kernel trace)

--gzip: the gzip FASTQ file alone (--quality random: qualities drawn from eight values, as a sequencer's, in place of a
constant line): the chunked device inflate of gap2seq_amd/csrc/gzip_inflate.hip asked for (G2S_DEVICE_GZIP=1) at chunks of 256 KiB
and of 1 MiB, the same build with the mode off (zlib), and --parent's library.

Needs a GPU."""
import argparse
import ctypes as C
import gzip
import json
import os
import resource
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCHES = ("G2S_HOST_BUILD", "G2S_HOST_READS", "G2S_HOST_INFLATE", "G2S_BUILD_PASS_KEYS", "G2S_BUILD_PIECE_BYTES",
            "G2S_BUILD_TEXT_FIRST_BYTES", "G2S_BUILD_RESIDENT_CAP", "G2S_BUILD_BAM_STREAM", "G2S_DEVICE_GZIP",
            "G2S_GZIP_CHUNK_BYTES", "G2S_GZIP_WINDOW_CHUNKS", "G2S_GZIP_SLOT_RATIO")


def bgzf(raw, out):
    for o in range(0, len(raw), 65280):
        payload = raw[o:o + 65280]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = c.compress(payload) + c.flush()
        out.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(cdata) + 25).to_bytes(2, "little") + cdata +
                  (zlib.crc32(payload) & 0xFFFFFFFF).to_bytes(4, "little") + len(payload).to_bytes(4, "little"))
    out.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


_HEX = bytes.maketrans(b"ACGTacgt", b"12481248")


def bam(lines, out):
    """the FASTA records of `lines` (header, sequence, header, ...) as unaligned BAM records: no reference, flag 4"""
    raw = [b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 0)]
    for i in range(0, len(lines) - 1, 2):
        name, seq = lines[i][1:].split()[0] + b"\0", lines[i + 1]
        # (two codes a byte, the first in the high nibble: the codes written as hexadecimal digits; anything else is N)
        digits = bytes(c if c in b"1248" else 102 for c in seq.translate(_HEX)) if seq.strip(b"ACGTacgt") else seq.translate(_HEX)
        packed = bytes.fromhex((digits + b"0" * (len(seq) & 1)).decode("ascii"))
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, len(seq), -1, -1, 0) + name + packed + b"\xff" * len(seq)
        raw.append(struct.pack("<i", len(body)) + body)
    bgzf(b"".join(raw), out)


def cut_reads(lines, length, k):
    """every sequence of `lines` (header, sequence, ...) as reads of `length` bases that overlap by k - 1: every k-mer of
    the sequence lies in one of them, so at solid 1 the graph is the uncut sequences'"""
    out = []
    for i in range(0, len(lines) - 1, 2):
        name, seq = lines[i].split()[0], lines[i + 1]
        for n, at in enumerate(range(0, max(len(seq) - k + 1, 1), length - k + 1)):
            out.append(name + b".%d" % n)
            out.append(seq[at:at + length])
    return out + [b""]


def write_files(config, d, with_bam=False, read_length=0, genome=0, only_gzip=False, quality="constant"):
    import bench
    from gap2seq_amd import lib as P
    genome_bp, k = bench.CONFIGS[config][:2]
    genome_bp = genome or genome_bp
    fa = P.G2S.synth_genome(genome_bp, 3, bench.GENOME_SEED).encode("ascii")
    lines = fa.split(b"\n")
    if read_length:  # (bench.py's read sets are a few sequences of the genome's length: short reads of the same k-mers)
        lines = cut_reads(lines, max(read_length, k), k)
        fa = b"\n".join(lines)
    if quality == "random":
        import random
        pool = bytes(random.Random(5).choices(b"FFFFF:,#", k=1 << 20))
        qual = lambda i, n: pool[(i * 7919) % ((1 << 20) - n):][:n] if n < (1 << 19) else (pool * (n // len(pool) + 1))[:n]
    else:
        qual = lambda i, n: b"I" * n
    fq = b"".join(b"@" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n+\n" + qual(i, len(lines[i + 1])) + b"\n"
                  for i in range(0, len(lines) - 1, 2))
    if only_gzip:
        path = os.path.join(d, "reads.fastq.gz")
        with gzip.GzipFile(path, "wb", compresslevel=6, mtime=0) as f:
            f.write(fq)
        return k, {"fastq.gz": path}
    paths = {f: os.path.join(d, "reads." + f) for f in ("fasta", "fastq", "fastq.gz", "bgzf.fastq.gz")}
    open(paths["fasta"], "wb").write(fa)
    open(paths["fastq"], "wb").write(fq)
    with gzip.GzipFile(paths["fastq.gz"], "wb", compresslevel=6, mtime=0) as f:
        f.write(fq)
    with open(paths["bgzf.fastq.gz"], "wb") as f:
        bgzf(fq, f)
    if with_bam:
        paths["bam"] = os.path.join(d, "reads.bam")
        with open(paths["bam"], "wb") as f:
            bam(lines, f)
    return k, paths


def child(library, path, k, threads):
    """one build in this process: a JSON line with its wall time, k-mers and resident set"""
    lib = C.CDLL(library)
    lib.g2s_graph_build_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.g2s_graph_num_kmers.restype = C.c_uint64
    lib.g2s_graph_num_kmers.argtypes = [C.c_void_p]
    lib.g2s_graph_free.argtypes = [C.c_void_p]
    lib.g2s_last_error.restype = C.c_char_p
    with tempfile.NamedTemporaryFile(suffix=".fa") as warm:
        warm.write(b">w\n" + b"ACGTTGCAAGGCTTAACCGGTATCGATCGGATTACAGGCATT" * 50 + b"\n")
        warm.flush()
        h = C.c_void_p()
        if lib.g2s_graph_build_files(warm.name.encode(), k, 1, threads, C.byref(h)) != 0:
            raise SystemExit("warm-up: " + (lib.g2s_last_error() or b"").decode())
        lib.g2s_graph_free(h)
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.g2s_graph_build_files(path.encode(), k, 1, threads, C.byref(h))
    wall = time.perf_counter() - t0
    if rc != 0:
        raise SystemExit("build: " + (lib.g2s_last_error() or b"").decode())
    out = dict(wall_s=wall, kmers=lib.g2s_graph_num_kmers(h), rss_mb=(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - rss0) / 1024.0)
    try:
        lib.g2s_test_last_reads_load.argtypes = [C.POINTER(C.c_uint64)] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_uint64,
                                                                               C.POINTER(C.c_uint64)]
        raw, pos, on = C.c_uint64(), C.c_uint64(), C.c_int()
        lib.g2s_test_last_reads_load(None, C.byref(raw), C.byref(pos), None, None, C.byref(on), None, 0, None)
        out.update(raw_bytes=raw.value, positions=pos.value, text_on_device=on.value)
        lib.g2s_test_last_reads_bam.argtypes = [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_int)] * 3
        files, kernels, reason, anomaly = C.c_uint64(), C.c_int(), C.c_int(), C.c_int()
        lib.g2s_test_last_reads_bam(C.byref(files), None, None, C.byref(kernels), C.byref(reason), C.byref(anomaly))
        if files.value:  # (a BAM file: whether the kernels wrote its text, and when not, why — include/g2s_test.h)
            out.update(bam_by_kernels=kernels.value, bam_reason=reason.value, bam_anomaly=anomaly.value)
            lib.g2s_test_last_reads_bam_stream.argtypes = [C.POINTER(C.c_uint64)] * 3
            streamed, windows, peak = C.c_uint64(), C.c_uint64(), C.c_uint64()
            lib.g2s_test_last_reads_bam_stream(C.byref(streamed), C.byref(windows), C.byref(peak))
            out.update(bam_streamed=streamed.value, bam_stream_windows=windows.value, bam_stream_peak=peak.value)
        lib.g2s_test_last_reads_gzip.argtypes = [C.POINTER(C.c_uint64)] * 6 + [C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        v = [C.c_uint64() for _ in range(7)]
        oc = C.c_int()
        lib.g2s_test_last_reads_gzip(*[C.byref(x) for x in v[:6]], C.byref(oc), C.byref(v[6]))
        if v[0].value:  # (the chunked device inflate was tried: include/g2s_test.h)
            out.update(gzip=dict(windows=v[1].value, chunks=v[2].value, starts_found=v[3].value, absorbed=v[4].value,
                                 members=v[5].value, outcome=oc.value, peak_device_bytes=v[6].value))
    except AttributeError:  # (the parent's library)
        pass
    lib.g2s_graph_free(h)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent", default="", help="the library of the commit before, for the uncompressed files")
    ap.add_argument("--bam", action="store_true", help="the BAM form: device route, streaming form, host loader, and --parent on BGZF FASTQ")
    ap.add_argument("--parent-bam", action="store_true", help="with --bam and --parent: the parent's library on the BAM file, both ways")
    ap.add_argument("--read-length", type=int, default=0, help="cut the sequences into reads of this length that overlap by k - 1")
    ap.add_argument("--gzip", action="store_true", help="the gzip FASTQ file alone: the chunked device inflate, zlib, and --parent")
    ap.add_argument("--genome", type=int, default=0, help="base pairs of the synthetic genome in place of the config's")
    ap.add_argument("--quality", default="constant", choices=["constant", "random"])
    ap.add_argument("--slot-ratio", type=int, default=0, help="G2S_GZIP_SLOT_RATIO of the device-gzip ways")
    ap.add_argument("--more-ways", action="store_true", help="--gzip: chunks of 64 KiB in windows of 512 and of 256 KiB in windows of 256 too")
    ap.add_argument("--chunk", type=int, default=0, help="--once gzip: G2S_GZIP_CHUNK_BYTES")
    ap.add_argument("--once", default="", help="one device-loader build of this form in this process, nothing else")
    ap.add_argument("--child", nargs=4, metavar=("LIBRARY", "PATH", "K", "THREADS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), int(args.child[3]))
        return 0
    here = os.path.join(ROOT, "gap2seq_amd", "libg2s_hip.so")
    with tempfile.TemporaryDirectory() as d:
        k, paths = write_files(args.config, d, args.bam or args.once in ("bam", "stream"), args.read_length, args.genome,
                               args.gzip, args.quality)
        sizes = {f: os.path.getsize(p) for f, p in paths.items()}
        if args.once:
            for name in SWITCHES:
                os.environ.pop(name, None)
            if args.once == "stream":  # (the BAM file through the streaming form)
                os.environ["G2S_BUILD_BAM_STREAM"] = "1"
            if args.once == "gzip":
                os.environ["G2S_DEVICE_GZIP"] = "1"
                if args.chunk:
                    os.environ["G2S_GZIP_CHUNK_BYTES"] = str(args.chunk)
                if args.slot_ratio:
                    os.environ["G2S_GZIP_SLOT_RATIO"] = str(args.slot_ratio)
            child(here, paths[{"stream": "bam", "gzip": "fastq.gz"}.get(args.once, args.once)], k, args.threads)
            return 0
        ways = []  # (name, form, library, switches)
        if args.bam:
            ways = [("stream bam", "bam", here, {"G2S_BUILD_BAM_STREAM": "1"}), ("device bam", "bam", here, {}),
                    ("host-reads bam", "bam", here, {"G2S_HOST_READS": "1"})]
            if args.parent and args.parent_bam:
                ways += [("parent device bam", "bam", args.parent, {}), ("parent host-reads bam", "bam", args.parent, {"G2S_HOST_READS": "1"})]
            elif args.parent:
                ways.append(("parent bgzf.fastq.gz", "bgzf.fastq.gz", args.parent, {}))
        if args.gzip:
            ratio = {"G2S_GZIP_SLOT_RATIO": str(args.slot_ratio)} if args.slot_ratio else {}
            ways = [("device-gzip 256K fastq.gz", "fastq.gz", here, dict(ratio, G2S_DEVICE_GZIP="1", G2S_GZIP_CHUNK_BYTES=str(256 << 10))),
                    ("device-gzip 1M fastq.gz", "fastq.gz", here, dict(ratio, G2S_DEVICE_GZIP="1", G2S_GZIP_CHUNK_BYTES=str(1 << 20))),
                    ("zlib fastq.gz", "fastq.gz", here, {})]
            for chunk, window in ([(64 << 10, 512), (256 << 10, 256)] if args.more_ways else []):
                ways.append(("device-gzip %dK x %d fastq.gz" % (chunk >> 10, window), "fastq.gz", here,
                             dict(ratio, G2S_DEVICE_GZIP="1", G2S_GZIP_CHUNK_BYTES=str(chunk), G2S_GZIP_WINDOW_CHUNKS=str(window))))
            if args.parent:
                ways.append(("parent fastq.gz", "fastq.gz", args.parent, {}))
        for f in ([] if args.bam or args.gzip else paths):
            ways.append(("device " + f, f, here, {}))
            ways.append(("host-reads " + f, f, here, {"G2S_HOST_READS": "1"}))
            if args.parent and not f.endswith(".gz"):
                ways.append(("parent " + f, f, args.parent, {}))
        if not args.bam and not args.gzip:
            ways.append(("device+zlib bgzf.fastq.gz", "bgzf.fastq.gz", here, {"G2S_HOST_INFLATE": "1"}))
        runs = {w[0]: [] for w in ways}
        for rep in range(args.reps):
            for name, form, library, switches in ways:
                env = {key: v for key, v in os.environ.items() if key not in SWITCHES}
                env.update(switches)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", library, paths[form], str(k), str(args.threads)],
                                     env=env, capture_output=True, text=True, timeout=900)
                if res.returncode != 0:
                    raise SystemExit("%s failed:\n%s%s" % (name, res.stdout, res.stderr))
                r = json.loads(res.stdout.strip().splitlines()[-1])
                runs[name].append(r)
                print("rep %d %-28s %.3f s, %7.0f MiB resident, %d k-mers %s" % (
                    rep, name, r["wall_s"], r["rss_mb"], r["kmers"], "(text on the device)" if r.get("text_on_device") else ""), flush=True)
    out = {"config": args.config, "k": k, "read_length": args.read_length, "file_bytes": sizes, "ways": {}}
    for name, rs in runs.items():
        ts = sorted(r["wall_s"] for r in rs)
        out["ways"][name] = dict(median_s=statistics.median(ts), min_s=ts[0], max_s=ts[-1], reps=len(ts), kmers=rs[0]["kmers"],
                                 rss_mb=statistics.median(r["rss_mb"] for r in rs), text_on_device=rs[0].get("text_on_device"),
                                 raw_bytes=rs[0].get("raw_bytes"), positions=rs[0].get("positions"),
                                 bam_by_kernels=rs[0].get("bam_by_kernels"), bam_reason=rs[0].get("bam_reason"),
                                 bam_streamed=rs[0].get("bam_streamed"), bam_stream_windows=rs[0].get("bam_stream_windows"),
                                 bam_stream_peak=rs[0].get("bam_stream_peak"), gzip=rs[0].get("gzip"))
    out["same_kmers"] = len({v["kmers"] for v in out["ways"].values()}) == 1
    print(json.dumps(out))
    return 0 if out["same_kmers"] else 1


if __name__ == "__main__":
    sys.exit(main())
