#!/usr/bin/env python3
"""Write tests/zstd_vectors.py: zstd frames made by the system libzstd (through ctypes; no other source), for the
codec tests to decode on machines that may have no zstd library.

The in-tree encoder (csrc/codec/zstd.cc) writes Raw literals and Predefined-mode sequences only, so Huffman
literals, described FSE tables, Repeat and RLE modes and Treeless literals reach the decoders through these
vectors. Every vector is (name, spec, level, checksum, content_size, frame): `spec` is the seed formula of its raw
bytes (raw_of(spec) in the written module regenerates them, so they are not stored), the frame is base64.
libzstd's own round trip is checked here, at generation time; the tests then check the decoders against raw_of.

Candidates are tried in order and kept when they add to the coverage the tests ask for (block types, literal types,
1 and 4 streams, weight encodings, every sequence mode for every table, a frame of three or more blocks, a match
reaching more than 128 KiB back), measured with native.zstd_decoder_stats; the fixed list at the end adds levels
1, 3, 9 and 19 with and without checksum and content size and the literal-section sizes the device tests want.

Usage: python tools/make_zstd_vectors.py   (needs libzstd.so.1 and the built package)
"""
from __future__ import annotations

import base64
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_SRC = '''
import random


def raw_of(spec) -> bytes:
    """The raw bytes of a vector from its seed formula."""
    kind = spec[0]
    if kind == "random":
        _, n, seed = spec
        return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""
    if kind == "byte":
        return bytes([spec[2]]) * spec[1]
    if kind == "uniform":  # n bytes uniform over k symbols: Huffman gains, matches are rare
        _, n, seed, k = spec
        rnd = random.Random(seed)
        return bytes(48 + rnd.getrandbits(16) % k for _ in range(n))
    if kind == "words":  # words of a vocabulary of `vocab` words, space separated, cut at n bytes
        _, n, seed, vocab = spec
        rnd = random.Random(seed)
        words = [bytes(97 + rnd.getrandbits(16) % 26 for _ in range(2 + rnd.getrandbits(16) % 8)) for _ in range(vocab)]
        out = bytearray()
        while len(out) < n:
            out += words[rnd.getrandbits(16) % vocab] + b" "
        return bytes(out[:n])
    if kind == "periodic":  # a random period repeated; every `noise` bytes one byte is replaced (0: never)
        _, n, period, seed, noise = spec
        rnd = random.Random(seed)
        base = rnd.getrandbits(8 * period).to_bytes(period, "little")
        out = bytearray((base * (n // period + 1))[:n])
        if noise:
            for at in range(noise, n, noise):
                out[at] = rnd.getrandbits(8)
        return bytes(out)
    if kind == "sprinkle":  # the same, one byte value at random distances of gap / 2 .. 3 gap / 2
        _, n, period, seed, gap, value = spec
        rnd = random.Random(seed)
        base = rnd.getrandbits(8 * period).to_bytes(period, "little")
        out = bytearray((base * (n // period + 1))[:n])
        at = 0
        while True:
            at += gap // 2 + rnd.getrandbits(16) % gap + 1
            if at >= n:
                return bytes(out)
            out[at] = value
    if kind == "low":  # n bytes uniform over the byte values 0 .. k - 1: equal code lengths, direct weights
        _, n, seed, k = spec
        rnd = random.Random(seed)
        return bytes(rnd.getrandbits(16) % k for _ in range(n))
    if kind == "cat":
        return b"".join(raw_of(s) for s in spec[1:])
    raise ValueError(kind)
'''
exec(GEN_SRC)  # raw_of, the same text the written module carries

LIB = ctypes.CDLL("libzstd.so.1")
for f in ("ZSTD_compressBound", "ZSTD_compress2", "ZSTD_decompress", "ZSTD_CCtx_setParameter"):
    getattr(LIB, f).restype = ctypes.c_size_t
LIB.ZSTD_createCCtx.restype = ctypes.c_void_p
LIB.ZSTD_isError.restype = ctypes.c_uint
ZSTD_c_compressionLevel, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 100, 200, 201


def compress(raw: bytes, level: int, checksum: bool, content_size: bool) -> bytes:
    cctx = ctypes.c_void_p(LIB.ZSTD_createCCtx())
    try:
        for k, v in ((ZSTD_c_compressionLevel, level), (ZSTD_c_contentSizeFlag, int(content_size)),
                     (ZSTD_c_checksumFlag, int(checksum))):
            assert not LIB.ZSTD_isError(ctypes.c_size_t(LIB.ZSTD_CCtx_setParameter(cctx, k, v)))
        cap = LIB.ZSTD_compressBound(ctypes.c_size_t(len(raw)))
        out = ctypes.create_string_buffer(cap)
        r = LIB.ZSTD_compress2(cctx, out, ctypes.c_size_t(cap), raw, ctypes.c_size_t(len(raw)))
        assert not LIB.ZSTD_isError(ctypes.c_size_t(r))
        frame = out.raw[:r]
    finally:
        LIB.ZSTD_freeCCtx(cctx)
    back = ctypes.create_string_buffer(max(len(raw), 1))
    r = LIB.ZSTD_decompress(back, ctypes.c_size_t(len(raw)), frame, ctypes.c_size_t(len(frame)))
    assert not LIB.ZSTD_isError(ctypes.c_size_t(r)) and back.raw[:r] == raw, "libzstd's own round trip"
    return frame


def features(st) -> set:
    f = set()
    for k, v in st["blocks"].items():
        if v:
            f.add("block:" + k)
    for k, v in st["literals"].items():
        if v:
            f.add("literals:" + k)
    for k, v in st["weights"].items():
        if v:
            f.add("weights:" + k)
    for t, modes in st["modes"].items():
        for k, v in modes.items():
            if v:
                f.add(f"mode:{t}:{k}")
    if st["max_frame_blocks"] >= 3:
        f.add("three-blocks")
    if st["max_offset"] > 128 * 1024:
        f.add("far-match")
    return f


WANTED = ({"block:raw", "block:rle", "block:compressed", "three-blocks", "far-match", "weights:direct", "weights:fse"} |
          {"literals:" + k for k in ("raw", "rle", "compressed", "treeless", "streams1", "streams4")} |
          {f"mode:{t}:{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")})

# (name, spec, level): kept only when they add coverage
CANDIDATES = [
    ("random", ("random", 3000, 1), 3),
    ("byte-300k", ("byte", 300000, 0x61), 3),
    ("few-sequences", ("words", 300, 2, 12), 3),
    ("tiny", ("words", 40, 3, 4), 3),
    ("far", ("cat", ("random", 2500, 5), ("periodic", 140000, 7, 6, 0), ("random", 2500, 5)), 3),
    ("small-alphabet", ("uniform", 3000, 7, 5), 1),
    ("direct-weights", ("low", 2000, 3, 4), 1),
    ("periodic-noise-wide", ("periodic", 30000, 200, 9, 50), 3),
    ("periodic-noise-200k", ("periodic", 200000, 200, 2, 50), 1),
    ("sprinkle-19", ("sprinkle", 140000, 40, 4, 50, 0x61), 19),
    ("words-140k-9", ("words", 140000, 11, 12), 9),
    ("words-140k-19", ("words", 140000, 13, 20), 19),
    ("words-140k-3", ("words", 140000, 11, 12), 3),
]
# always kept: (name, spec, level, checksum, content_size)
FIXED = [(f"words-l{lvl}-{'sum' if cs else 'nosum'}-{'fcs' if fc else 'nofcs'}", ("words", 6000, 20 + lvl, 60), lvl, cs, fc)
         for lvl in (1, 3, 9, 19) for cs, fc in ((False, False), (True, True), (True, False), (False, True))]
# literal sections of exactly these sizes, all literals and no sequence (the seeds are searched for that below)
LITERAL_SIZES = (255, 256, 1023, 1024, 1025, 1026)


def main() -> int:
    from uda_amd._native import native

    n = native()
    vectors, have = [], set()
    for name, spec, level in CANDIDATES:
        raw = raw_of(spec)
        frame = compress(raw, level, False, False)
        st = n.zstd_decoder_stats(frame, len(raw))
        new = (features(st) & WANTED) - have
        if new:
            have |= new
            vectors.append((name, spec, level, False, False, frame))
            print(f"{name}: {len(raw)} -> {len(frame)} adds {sorted(new)}")
    for name, spec, level, cs, fc in FIXED:
        vectors.append((name, spec, level, cs, fc, compress(raw_of(spec), level, cs, fc)))
    for size in LITERAL_SIZES:
        for seed in range(100, 200):
            spec = ("uniform", size, seed, 40)
            frame = compress(raw_of(spec), 1, False, False)
            st = n.zstd_decoder_stats(frame, size)
            if st["sequences"] == 0 and st["literals"]["compressed"] == 1 and st["blocks"]["compressed"] == 1:
                vectors.append((f"literals-{size}", spec, 1, False, False, frame))
                break
        else:
            raise SystemExit(f"no seed gives a literal section of {size} bytes")
    missing = WANTED - have
    print("missing:", sorted(missing))
    lines = ['"""zstd frames written by libzstd 1.4.8 (tools/make_zstd_vectors.py): generated, do not edit.',
             "", "VECTORS: (name, spec, level, checksum, content_size, frame). raw_of(spec) regenerates the raw bytes.",
             '"""', "import base64", GEN_SRC, "", "VECTORS = ["]
    for name, spec, level, cs, fc, frame in vectors:
        b64 = base64.b64encode(frame).decode()
        chunks = [b64[i:i + 100] for i in range(0, len(b64), 100)] or [""]
        lines.append(f"    ({name!r}, {spec!r}, {level}, {cs}, {fc}, base64.b64decode(")
        lines += [f"        {c!r}" for c in chunks]
        lines.append("    )),")
    lines.append("]")
    path = os.path.join(ROOT, "tests", "zstd_vectors.py")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(path, os.path.getsize(path), "bytes,", len(vectors), "vectors")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
