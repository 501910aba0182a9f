"""LZ4 block-format streams built by hand from the format (not by our encoder), and a small pure-Python
decoder. No LZ4 library is available to the tests, so these are the independent oracle: the vectors
check the decoders, the Python decoder checks what the encoder emits.

  sequence := token, [literal-length extension], literals, offset (2 bytes LE), [match-length extension]
  token    := literal length << 4 | (match length - 4)
  a nibble of 15 is followed by extension bytes: each 255 adds 255, the first byte below 255 ends the run
  the last sequence ends after its literals (no offset); a block may end with the lone token 0x00
"""
A15 = bytes(range(65, 80))                      # 15 literals
L100 = bytes((7 * i + 3) & 0xFF for i in range(100))
L200 = bytes((5 * i + 1) & 0xFF for i in range(200))
L270 = bytes((3 * i) & 0xFF for i in range(270))
L273 = bytes((11 * i + 2) & 0xFF for i in range(273))
L65535 = bytes((i * i + (i >> 8)) & 0xFF for i in range(65535))


def _fill(seed: bytes, n: int) -> bytes:
    """What a match of length n at offset len(seed) appends after `seed`."""
    out = bytearray(seed)
    for _ in range(n):
        out.append(out[-len(seed)])
    return bytes(out[len(seed):])


VECTORS = [
    # (name, stream, expected output)
    ("literals_only", b"\x30abc", b"abc"),
    ("empty", b"\x00", b""),
    # 1 literal, match length 10 at offset 1 (period-1 fill, length > offset), then the lone end token
    ("offset1_fill", b"\x16a" + b"\x01\x00" + b"\x00", b"a" * 11),
    ("offset_equals_length", b"\x40abcd" + b"\x04\x00" + b"\x00", b"abcdabcd"),
    # match length 100 = 4 + 15 + 81 at offset 3, then one literal
    ("offset_below_length_over_64", b"\x3fabc" + b"\x03\x00" + b"\x51" + b"\x10Z", b"abc" + _fill(b"abc", 100) + b"Z"),
    ("literal_run_15", b"\xf0\x00" + A15, A15),
    ("literal_run_270", b"\xf0\xff\x00" + L270, L270),
    ("literal_run_273", b"\xf0\xff\x03" + L273, L273),
    # match length 19 = 4 + 15 + 0
    ("match_length_19", b"\x4fabcd" + b"\x04\x00" + b"\x00" + b"\x00", b"abcd" + _fill(b"abcd", 19)),
    # match length 281 = 4 + 15 + 255 + 7 at offset 2, then two literals
    ("match_length_ff_extension", b"\x2fxy" + b"\x02\x00" + b"\xff\x07" + b"\x20!?", b"xy" + _fill(b"xy", 281) + b"!?"),
    # 100 literals = 15 + 85: the vector-copy path of the device decoder
    ("literal_run_over_64", b"\xf0\x55" + L100, L100),
    # 200 literals = 15 + 185, then match length 40 = 4 + 15 + 21 at offset 150, then 3 literals
    ("offset_over_64_short_match", b"\xff\xb9" + L200 + b"\x96\x00" + b"\x15" + b"\x30end", L200 + L200[50:90] + b"end"),
    # 65535 literals = 15 + 256 * 255 + 240, then match length 8 at the largest offset
    ("offset_65535", b"\xf4" + b"\xff" * 256 + b"\xf0" + L65535 + b"\xff\xff" + b"\x00", L65535 + L65535[:8]),
]


def hadoop_block(raw: bytes, payload: bytes) -> bytes:
    """Hadoop BlockCompressorStream framing: [u32 BE raw][u32 BE compressed][payload]."""
    return len(raw).to_bytes(4, "big") + len(payload).to_bytes(4, "big") + payload


def lz4_walk(data: bytes):
    """Pure-Python LZ4 block decoder. Returns (output, sequences) with one (literal length, match start in
    the output, offset, match length) per sequence; the last has offset 0 and match length 0. Raises
    ValueError on anything the format does not allow."""
    out, seqs, ip = bytearray(), [], 0

    def length(nibble):
        nonlocal ip
        n = nibble
        while nibble == 15:
            if ip >= len(data):
                raise ValueError("input ends in a length extension")
            b = data[ip]
            ip += 1
            n += b
            if b != 255:
                break
        return n

    while True:
        if ip >= len(data):
            raise ValueError("input ends where a token is due")
        token = data[ip]
        ip += 1
        lit = length(token >> 4)
        if ip + lit > len(data):
            raise ValueError("literals run past the input")
        out += data[ip:ip + lit]
        ip += lit
        if ip == len(data):
            seqs.append((lit, len(out), 0, 0))
            return bytes(out), seqs
        if ip + 2 > len(data):
            raise ValueError("input ends in an offset")
        off = data[ip] | data[ip + 1] << 8
        ip += 2
        if off == 0 or off > len(out):
            raise ValueError("bad offset")
        mlen = length(token & 15) + 4
        seqs.append((lit, len(out), off, mlen))
        for _ in range(mlen):
            out.append(out[-off])


def lz4_block_decode(data: bytes) -> bytes:
    return lz4_walk(data)[0]
