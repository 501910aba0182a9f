"""zstd map outputs (Hadoop's ZStandardCodec) on the host: zstd_decompress and the incremental ZstdDecoder behind
BlockDecoder / host_decode_partition on the frames of tests/zstd_cases.py and tests/zstd_vectors.py (which libzstd
has judged or written: tests/test_zstd_cases_cpu.py), trailer detection, the in-tree encoder against our decoder
and, where it loads, libzstd, the codec resolvers, the MOF writer, reduce tasks on the CPU backend, and the codec's
stand-alone sanitizer program."""
import collections
import os
import random
import struct
import zlib

import pytest

from tests import zstd_cases as zc
from tests.test_zstd_cases_cpu import LIB, lib_compress, lib_decompress, live
from tests.zstd_vectors import VECTORS, raw_of
from uda_amd.utils import datagen

ZSTD = 6
ZSTD_CLASS = "org.apache.hadoop.io.compress.ZStandardCodec"
WINDOW_LIMIT = 128 << 20
BLOCK = 128 * 1024


def all_valid():
    """[(name, stream, raw)]: the hand-built cases and the libzstd-written vectors."""
    return zc.VALID + zc.SHAPES + zc.BEYOND_WINDOW + [(v[0], v[5], raw_of(v[1])) for v in VECTORS]


@pytest.fixture(scope="module")
def valid():
    return all_valid()


def window_of(stream):
    """Window_Size of a stream's first frame (skippable frames skipped); None if there is none."""
    at = 0
    while stream[at:at + 4] != zc.MAGIC:
        if len(stream) - at < 8 or struct.unpack_from("<I", stream, at)[0] & 0xFFFFFFF0 != 0x184D2A50:
            return None
        at += 8 + struct.unpack_from("<I", stream, at + 4)[0]
    d = stream[at + 4]
    if d & 0x20:
        n = 1 if d >> 6 == 0 else 1 << (d >> 6)
        skip = (0, 1, 2, 4)[d & 3]
        v = int.from_bytes(stream[at + 5 + skip:at + 5 + skip + n], "little")
        return v + 256 if n == 2 else v
    w = stream[at + 5]
    base = 1 << (10 + (w >> 3))
    return base + (base >> 3) * (w & 7)


def ifile_crc(stream):
    return struct.pack(">I", zlib.crc32(stream))


def sequence_steered(nseq, seed=5):
    """Raw bytes that the in-tree encoder turns into exactly `nseq` sequences in one block: 255 distinct four-byte
    words [j, 0, 0, 0] as literals, then words drawn so that no pair of neighbours occurs twice (nor in the
    dictionary's order), so every word is one match of four bytes with no literal ahead of it."""
    rnd = random.Random(seed)
    out = bytearray()
    for j in range(1, 256):
        out += bytes([j, 0, 0, 0])
    used = {(j, j + 1) for j in range(1, 255)}
    cur = 255
    for _ in range(nseq):
        while True:
            k = 1 + rnd.getrandbits(16) % 255
            if (cur, k) not in used:
                break
        used.add((cur, k))
        out += bytes([k, 0, 0, 0])
        cur = k
    return bytes(out)


def encoder_inputs():
    tera = b"".join(datagen.streams(datagen.terasort(num_maps=1, reducers=1, rows_per_map=2500, seed=3))[0])
    words = b"".join(datagen.streams(datagen.wordcount(num_maps=1, reducers=1, words_per_map=20000, seed=4))[0])
    rnd = random.Random(8)
    return {
        "empty": b"", "one-byte": b"z", "repeated-byte": b"\x07" * 300000, "two-bytes": b"ab",
        "incompressible": rnd.getrandbits(8 * 70000).to_bytes(70000, "little"),
        "terasort": tera, "wordcount": words,
        "seq-127": sequence_steered(127), "seq-128": sequence_steered(128),
        "seq-0x7f00": sequence_steered((BLOCK - 1020) // 4)[:BLOCK],
    }


@pytest.fixture(scope="module")
def encoded(native):
    return {name: (native.zstd_compress(raw), raw) for name, raw in encoder_inputs().items()}


def test_one_shot_decodes_every_valid_frame(native, valid):
    for name, stream, raw in valid:
        out, used = native.zstd_decompress(stream, len(raw))
        assert out == raw and used == len(stream), name
        if raw:
            with pytest.raises(ValueError):
                native.zstd_decompress(stream, len(raw) - 1)


@pytest.mark.parametrize("case", zc.INVALID + zc.STRICTER, ids=lambda c: c[0])
def test_one_shot_refuses_the_invalid_cases(native, case):
    name, stream, cap = case
    with pytest.raises(ValueError, match="corrupt zstd frame"):
        native.zstd_decompress(stream, cap)


def test_refusals_are_by_name(native):
    by = dict((c[0], c[1]) for c in zc.INVALID)
    for name, what in (("dictionary-id", "needs a dictionary"), ("wrong-magic", "wrong magic"),
                       ("reserved-descriptor-bit", "reserved descriptor bit"), ("reserved-block-type", "reserved block type"),
                       ("fcs-mismatch-more", "content size"), ("checksum-mismatch", "content checksum mismatch"),
                       ("offset-before-start", "before the frame's first byte"),
                       ("treeless-first-block", "Treeless"), ("weights-incomplete", "do not complete a tree"),
                       ("fse-description-overshoots", "FSE table description"),
                       ("oversize-compressed-block", "block larger")):
        with pytest.raises(ValueError, match=what):
            native.zstd_decompress(by[name], 1 << 18)


def test_mutated_vectors_are_refused_or_decode_to_the_same_bytes(native):
    """Single flipped bits in frames that carry a content checksum. A flip is either refused (by the format or by
    the checksum) or lands in a bit no decoder reads, and then the frame still decodes to exactly its bytes; a
    frame is never taken with other bytes. Where libzstd loads and takes a mutated frame too, the bytes agree
    with its as well. (Which frames each refuses may differ: docs/ARCHITECTURE.md lists the known differences.)"""
    rnd = random.Random(77)
    taken = refused = 0
    for name, spec, level, checksum, content_size, frame in VECTORS:
        if not checksum:
            continue
        raw = raw_of(spec)
        for _ in range(12):
            mut = bytearray(frame)
            mut[5 + rnd.getrandbits(16) % (len(mut) - 5)] ^= 1 << rnd.getrandbits(3)
            mut = bytes(mut)
            try:
                out, used = native.zstd_decompress(mut, len(raw))
            except ValueError:
                refused += 1
                continue
            taken += 1
            assert out == raw, name
            if LIB is not None:
                ref = lib_decompress(mut, len(raw))
                assert ref is None or ref == out, name
    assert refused > 10 * taken  # (nearly every bit of a frame matters)


BEYOND = {c[0] for c in zc.BEYOND_WINDOW}


def incremental_refusal(name, stream):
    """What the incremental decoder says to a valid frame it does not take, or None: a window above its limit, and
    an offset beyond Window_Size, which the one-shot decoder takes as libzstd's one-shot call does."""
    if window_of(stream) > WINDOW_LIMIT:
        return "Window_Size above 128 MiB"
    return "offset beyond Window_Size" if name in BEYOND else None


@pytest.mark.parametrize("piece", [1, 7, 4096])
def test_incremental_decoder_in_pieces(native, valid, piece):
    for name, stream, raw in valid:
        if piece == 1 and len(stream) > 40000:
            continue  # (the same frames go through at 7 and 4096; byte-wise feeding of these is slow, not different)
        refusal = incremental_refusal(name, stream)
        if refusal:
            with pytest.raises(ValueError, match=refusal):
                native.zstd_stream_decode(stream, piece)
            continue
        out, consumed, finished, most, most_in = native.zstd_stream_decode(stream, piece)
        assert out == raw and finished and consumed == len(stream), name
        # history and output: Window_Size and one block (a block is at most min(window, 128 KiB)), exactly
        window = window_of(stream)
        assert most <= window + min(window, BLOCK), (name, most)
        # input: a block with its header, a frame header or checksum ahead of it, the piece just fed; the vector
        # grows in 4 KiB steps
        assert most_in <= 3 + BLOCK + 18 + piece + 4096, (name, most_in)


def test_incremental_decoder_memory_is_bounded_by_the_window(native):
    """3 MB of output through a 1 KiB window: the history stays at window + one block, however long the frame is."""
    block = zc.rle_block(0x11, 1024)
    stream = zc.frame([block] * 3000 + [zc.raw_block(b"end", True)], window=(0, 0))
    out, consumed, finished, most, most_in = native.zstd_stream_decode(stream, 4096)
    assert out == b"\x11" * (1024 * 3000) + b"end" and finished and consumed == len(stream)
    assert most <= 1024 + 1024, most
    assert most_in <= 2 * 4096, most_in  # (what a 4 KiB feed leaves undecoded plus the next feed)
    # and with the largest blocks: 2 MiB through a 128 KiB window
    big = zc.frame([zc.rle_block(7, BLOCK)] * 16 + [zc.raw_block(b"", True)], window=(7, 0))
    out, consumed, finished, most, most_in = native.zstd_stream_decode(big, 4096)
    assert out == b"\x07" * (16 * BLOCK) and finished and most <= 2 * BLOCK, most


def test_incremental_decoder_refuses_the_invalid_cases(native):
    for name, stream, cap in zc.INVALID + zc.STRICTER:
        for piece in (1, 7, 4096):
            try:
                out, consumed, finished, _, _ = native.zstd_stream_decode(stream, piece)
            except ValueError:
                continue
            assert not finished, (name, piece)  # (a truncated frame never ends)


def test_block_decoder_and_the_trailer_rule(native, valid):
    """The frame alone, with a correct IFile checksum behind it, and with four zero bytes behind it."""
    for name, stream, raw in valid:
        if incremental_refusal(name, stream):
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(ZSTD, stream)
            continue
        for chunk in (1 if len(stream) < 3000 else 1000, 4096):
            assert native.block_decompress(ZSTD, stream, chunk) == raw, name
        assert native.host_decode_partition(ZSTD, stream) == (raw, 0), name
        for tail in (ifile_crc(stream), b"\x00\x00\x00\x00"):
            out, used = native.zstd_decompress(stream + tail, len(raw))
            assert out == raw and used == len(stream), name
            assert native.host_decode_partition(ZSTD, stream + tail) == (raw, 4), name


def test_host_decode_partition_refuses_other_tails(native):
    stream = zc.frame([zc.raw_block(b"hello", True)])
    assert native.host_decode_partition(ZSTD, stream) == (b"hello", 0)
    assert native.host_decode_partition(ZSTD, stream + b"\x00" * 4) == (b"hello", 4)
    for tail in (b"\x00", b"\x00" * 3, b"\x00" * 5):
        with pytest.raises((ValueError, RuntimeError)):
            native.host_decode_partition(ZSTD, stream + tail)
    with pytest.raises((ValueError, RuntimeError)):
        native.host_decode_partition(ZSTD, stream[:-1])


def test_encoder_round_trips(native, encoded):
    for name, (frame, raw) in encoded.items():
        out, used = native.zstd_decompress(frame, len(raw))
        assert out == raw and used == len(frame), name
        out, consumed, finished, _, _ = native.zstd_stream_decode(frame, 4096)
        assert out == raw and finished and consumed == len(frame), name
        d = frame[4]
        assert frame[:4] == zc.MAGIC and d == 0, name  # no content size, no checksum, no dictionary id


@live
def test_libzstd_decodes_what_the_encoder_writes(encoded):
    for name, (frame, raw) in encoded.items():
        assert lib_decompress(frame, len(raw)) == raw, name


def test_encoder_really_compresses(native, encoded):
    """Compressed blocks throughout and fewer bytes than went in. How much fewer is left open for the TeraSort
    records: most of a record here is random letters, which only entropy-coded literals would shrink and this
    encoder writes Raw literals; wordcount's words recur, so at least a third must go; a repeated byte costs
    four bytes a block."""
    for name, most in (("terasort", 1.0), ("wordcount", 2 / 3), ("repeated-byte", 0.001)):
        frame, raw = encoded[name]
        assert len(frame) < most * len(raw), (name, len(frame), len(raw))
        st = native.zstd_decoder_stats(frame, len(raw))
        assert st["blocks"]["raw"] == 0, (name, st)
    assert native.zstd_decoder_stats(encoded["repeated-byte"][0], 300000)["blocks"]["rle"] == 3
    frame, raw = encoded["incompressible"]
    assert len(frame) <= len(raw) + 16 and native.zstd_decoder_stats(frame, len(raw))["blocks"] == {"raw": 1, "rle": 0, "compressed": 0}


def test_encoder_reaches_the_three_sequence_count_encodings(native, encoded):
    for name, want in (("seq-127", 127), ("seq-128", 128), ("seq-0x7f00", None)):
        frame, raw = encoded[name]
        st = native.zstd_decoder_stats(frame, len(raw))
        assert st["blocks"] == {"raw": 0, "rle": 0, "compressed": 1}, (name, st)
        if want is None:
            assert st["sequences"] >= 0x7F00, st
        else:
            assert st["sequences"] == want, st
        assert st["literals"]["raw"] == 1 and st["modes"]["ll"]["predefined"] == 1, st


def test_the_three_codec_resolvers(native):
    pkg = "org.apache.hadoop.io.compress."
    assert native.job_codec(ZSTD_CLASS) == 6
    for cls in (pkg + "GzipCodec", pkg + "DefaultCodec", pkg + "DeflateCodec", pkg + "SnappyCodec",
                "com.hadoop.compression.lzo.LzoCodec", pkg + "Lz4Codec", "", "null", pkg + "BZip2Codec", "no.such.Codec"):
        assert native.job_codec(cls) == native.map_output_codec(cls), cls
    assert native.job_codec(pkg + "BZip2Codec") == -1
    assert native.map_output_codec(ZSTD_CLASS) == -1 and native.codec_from_class(ZSTD_CLASS) == -1  # (pinned answers)


def test_zstd_is_no_block_codec(native):
    with pytest.raises((ValueError, RuntimeError)):
        native.block_compress(ZSTD, b"abc", 4096)
    with pytest.raises((ValueError, RuntimeError)):
        native.plan_block_streams(ZSTD, native.zstd_compress(b"abc" * 100))


def test_zstd_mof_tables(native):
    from uda_amd.utils.mof import CODEC_CLASSES, CODECS, encode_partitions
    assert CODECS["zstd"] == 6
    assert CODEC_CLASSES["zstd"] == ZSTD_CLASS
    assert (CODECS["zlib"], CODECS["gzip"], CODECS["lz4"]) == (4, 5, 3)
    parts = [b"first partition " * 50, b"", b"third"]
    for checksum in (False, True):
        data, index = encode_partitions(parts, "zstd", checksum=checksum)
        assert [r for _, r, _ in index] == [len(p) for p in parts]
        for (start, raw, plen), p in zip(index, parts):
            body = data[start:start + plen]
            assert body[:4] == zc.MAGIC
            if checksum:
                assert body[-4:] == struct.pack(">I", zlib.crc32(body[:-4]))
                body = body[:-4]
            assert native.zstd_decompress(body, len(p)) == (p, len(body))
        assert sum(plen for _, _, plen in index) == len(data)


def sorted_records(maps, partition):
    return sorted((kv for m in maps for kv in m[partition]), key=datagen.sort_key(datagen.TEXT))


def same_records(recs, want):
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert collections.Counter(recs) == collections.Counter(want)


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
@pytest.mark.parametrize("where", ["memory", "file"])
def test_zstd_loopback_reduce_cpu_backend(tmp_path, where, checksum):
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import encode_partitions, write_mof
    p = UdaProvider()
    try:
        job = "job_1_06%d%d" % (where == "file", checksum)
        maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=9)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            if where == "file":
                path, _ = write_mof(str(tmp_path), mid, parts, codec="zstd", checksum=checksum)
                p.add_mof_file(job, mid, path)
            else:
                p.add_mof_memory(job, mid, *encode_partitions(parts, "zstd", checksum=checksum))
            ids.append(mid)
        for max_buf_kb in (16, 1024):
            recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", max_buf_kb=max_buf_kb, kv_buf_size=8192)
            same_records(recs, sorted_records(maps, 0))
            assert c.failure is None and st["finished"]
            assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    finally:
        p.close()


def vector_partitions(parts, checksum, frames_of):
    data, index = bytearray(), []
    for p in parts:
        body = frames_of(p)
        if checksum:
            body += struct.pack(">I", zlib.crc32(body))
        index.append((len(data), len(p), len(body)))
        data += body
    return bytes(data), index


@live
@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
@pytest.mark.parametrize("shape", ["libzstd-checksummed", "two-frames"])
def test_zstd_partitions_libzstd_wrote_cpu_backend(checksum, shape):
    """Partitions as libzstd writes them (Huffman literals, described tables), and every partition as two frames
    with a skippable frame between: the host decoders take both."""
    from uda_amd.bridge import UdaProvider, run_reduce
    p = UdaProvider()
    try:
        job = "job_1_07%d%d" % (shape == "two-frames", checksum)
        maps = datagen.wordcount(num_maps=5, reducers=1, words_per_map=3000, seed=21)
        if shape == "two-frames":
            def frames_of(part):
                cut = len(part) // 3
                return lib_compress(part[:cut]) + zc.skippable(b"between") + lib_compress(part[cut:], 9)
        else:
            def frames_of(part):
                return lib_compress(part, 5)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            p.add_mof_memory(job, mid, *vector_partitions(parts, checksum, frames_of))
            ids.append(mid)
        recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", max_buf_kb=16, kv_buf_size=8192)
        same_records(recs, sorted_records(maps, 0))
        assert c.failure is None and st["finished"]
        assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    finally:
        p.close()


def test_zstd_corrupt_partition_fails_the_cpu_task_once(tmp_path):
    from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        job = "job_1_0770"
        maps = datagen.wordcount(num_maps=3, reducers=1, words_per_map=3000, seed=4)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            path, index = write_mof(str(tmp_path), mid, parts, codec="zstd")
            if i == 1:
                with open(path, "r+b") as f:
                    f.seek(4)
                    f.write(b"\x08")  # the reserved descriptor bit
            p.add_mof_file(job, mid, path)
            ids.append(mid)
        c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, codec="zstd", max_buf_kb=16,
                        conf={"mapred.uda.ifile.checksum": "off"})
        for m in ids:
            c.fetch("h", job, m, 0)
        with pytest.raises(UdaFallback, match="zstd") as e:
            c.wait(60)
        c.close()
        assert c.failure_calls == 1
        assert ids[1] in str(e.value), str(e.value)
    finally:
        p.close()


@pytest.mark.parametrize("delta", [-1, 1])
def test_zstd_index_raw_length_is_held_against_the_decoded_bytes_without_trailers(delta):
    """No trailer, so the frame's last block is handed out after the held-back bytes are fed: the task still fails
    on a length that is not the index's, with the last bytes, not after them."""
    from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider
    from uda_amd.utils.mof import encode_partitions
    p = UdaProvider()
    try:
        job = "job_1_079%d" % (delta > 0)
        maps = datagen.wordcount(num_maps=3, reducers=1, words_per_map=3000, seed=6)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            data, index = encode_partitions(parts, "zstd")
            if i == 1:
                index = [(start, raw + delta, plen) for start, raw, plen in index]
            p.add_mof_memory(job, mid, data, index)
            ids.append(mid)
        c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, codec="zstd", max_buf_kb=16)
        for m in ids:
            c.fetch("h", job, m, 0)
        with pytest.raises(UdaFallback, match="decodes to .* bytes, its index says") as e:
            c.wait(60)
        c.close()
        assert c.failure_calls == 1 and ids[1] in str(e.value), str(e.value)
    finally:
        p.close()


def test_init_accepts_zstandard_and_still_refuses_bzip2():
    from uda_amd.bridge import UdaConsumer
    c = UdaConsumer(1, "job_1_0780", "attempt_job_1_0780_r_000000_0", datagen.TEXT, codec=ZSTD_CLASS)
    c.close()
    with pytest.raises(Exception, match="unsupported compression codec"):
        c = UdaConsumer(1, "job_1_0781", "attempt_job_1_0781_r_000000_0", datagen.TEXT,
                        codec="org.apache.hadoop.io.compress.BZip2Codec")
        c.close()


def test_zstd_native_selftest_under_sanitizers(tmp_path, valid, encoded):
    """tests/native/zstd_selftest.cc, a program of its own, built with csrc/codec/zstd.cc under ASan + UBSan, over
    the valid and invalid cases and the vectors dumped here, their prefixes and mutations, and the encoder. Exit
    status 0 = no report, no disagreement. Nothing is loaded into Python under a sanitizer."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    cases = tmp_path / "cases"
    cases.mkdir()
    lines = []

    def dump(kind, name, stream, want=None):
        (cases / (name + ".in")).write_bytes(stream)
        if want is not None:
            (cases / (name + ".out")).write_bytes(want)
        lines.append(kind + " " + name)

    for name, stream, want in valid:
        dump("W" if incremental_refusal(name, stream) else "V", name, stream, want)
    for name, (frame, raw) in encoded.items():
        dump("V", "enc_" + name, frame, raw)
    for name, stream, cap in zc.INVALID + zc.STRICTER:
        dump("I", name, stream)
    (cases / "manifest").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "zstd_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc", "include"), os.path.join(root, "tests", "native", "zstd_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "zstd.cc"), "-o", exe], check=True)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout
