"""Block-decode cases assembled token by token, with pure-Python decoders as the oracle.

Nothing here comes from the project's encoders or decoders: a stream is put together from the format's
token layouts (LZO1X as lzo1x_d.ch reads it, Snappy's raw format, the LZ4 block format), its expected
output is what the assembler copied while it emitted the tokens, and the decoders below parse the bytes
again from the format alone. The assemblers keep the LZO1X state (0 after a match without trailing
literals, 1..3 after that many trailing literals, 4 after a literal run), so a token is only emitted where
the format allows it, and record for every token its chunk-relative input offset and its output offset.

The families place tokens on the edges of the device kernels (csrc/gpu/decode.hip); every offset is derived
from native.gpu_decode_geometry(), passed in as `geom`:

  reg_window / reg_align   the 256-byte register window, based at ip & ~3, refilled when a read crosses it
  lds_window / lds_align   the 2048-byte LDS window, based at ip & ~15
  short_copy               copies of up to 64 bytes are one masked byte move per lane (lean parse)
  vec_bytes / wave_step    wave_copy moves 16 bytes per lane, 1024 per wave step, then a byte tail
  lane_word                the lane parse reads its input 8 bytes at a time
  waves_per_block          blocks decoded by one workgroup
  prefix_slot              the slot of the production prefix decode

A window edge sits where the test says only if the window was based where the test thinks: the pads are
literal runs longer than short_copy (they are copied from memory and leave the window alone) between small
anchor tokens at the multiples of reg_window, so the register window steps from multiple to multiple, and
batch() starts every stream at a chosen address modulo lds_align, so chunk offsets are window offsets in the
kernels that base their window on the address.
"""
import random
import struct
import zlib
from collections import namedtuple

from tests.lz4_vectors import lz4_walk

CODECS = ("lzo", "snappy", "lz4")
CODEC_ID = {"snappy": 1, "lzo": 2, "lz4": 3}
LZO_MARKER = b"\x11\x00\x00"

# kind: token kind; ip: chunk-relative offset of its first byte; op: chunk-relative output offset; size: bytes
# of the token without literal payload; state: LZO state before it (0 elsewhere); trail: literals it carries
Tok = namedtuple("Tok", "kind ip op size state dist length trail")
# stream: Hadoop-framed blocks; raw: the whole expected output; braws: expected output per non-empty block
Case = namedtuple("Case", "name codec stream raw braws toks tag")
# chunk: the malformed chunk and cap its block's announced size (None: only the framing is wrong)
Corrupt = namedtuple("Corrupt", "name codec stream chunk cap")

LITERAL_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025, 1039, 1040, 2049)
MATCH_OFFSETS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 2048, 2049, 3072, 16383, 16384, 16385,
                 49151)
MATCH_LENGTHS = (2, 3, 4, 8, 9, 33, 34, 63, 64, 65, 66, 1024, 1030)
RUN_BYTES = (0, 1, 2, 5)


def prefix_clips(geom):
    """1, the 11 key bytes production reads from a slot, and both sides of short_copy and of the slot."""
    sc, slot = geom["short_copy"], geom["prefix_slot"]
    return (1, 11, sc - 1, sc, sc + 1, slot - 1, slot, slot + 1)


def _seed(name):
    return zlib.crc32(name.encode())


def _extend(out, dist, n):
    """LZ77 copy: n bytes from dist back, overlapping allowed."""
    if dist <= 0 or dist > len(out):
        raise ValueError("match reaches before the start of the output")
    start = len(out) - dist
    if dist >= n:
        out += out[start:start + n]
    else:
        pat = bytes(out[start:])
        out += (pat * (n // dist + 1))[:n]


# ---------------------------------------------------------------------------------------------- oracles
def lzo_decode(src):
    """LZO1X chunk -> bytes. ValueError on anything lzo1x_decompress_safe refuses."""
    out, n, ip, state = bytearray(), len(src), 0, 0

    def byte():
        nonlocal ip
        if ip >= n:
            raise ValueError("input ends inside a token")
        ip += 1
        return src[ip - 1]

    def run(base):  # zero-run length extension: 255 per zero byte, then a byte of 1..255
        t = 0
        while True:
            b = byte()
            if b:
                return t + base + b
            t += 255

    def literal(k):  # every literal copy leaves room for the 3-byte end marker
        nonlocal ip
        if ip + k + 3 > n:
            raise ValueError("literals run into the last three bytes")
        out.extend(src[ip:ip + k])
        ip += k

    if n and src[0] > 17:
        k = byte() - 17
        literal(k)
        state = k if k < 4 else 4
    while True:
        t = byte()
        if t < 16:
            if state == 0:
                literal(t + 3 if t else run(15) + 3)
                state = 4
                continue
            b = byte()
            dist, length, trail = (t >> 2) + (b << 2) + (2049 if state == 4 else 1), 3 if state == 4 else 2, t & 3
        elif t >= 64:
            dist, length, trail = 1 + ((t >> 2) & 7) + (byte() << 3), (t >> 5) + 1, t & 3
        else:
            mask = 31 if t >= 32 else 7
            length = (t & mask) + 2 if t & mask else run(mask) + 2
            v = byte()
            v |= byte() << 8
            trail = v & 3
            if t >= 32:
                dist = 1 + (v >> 2)
            else:
                d = ((t & 8) << 11) + (v >> 2)
                if d == 0:
                    if length != 3 or ip != n:
                        raise ValueError("malformed end marker")
                    return bytes(out)
                dist = 16384 + d
        _extend(out, dist, length)
        literal(trail)
        state = trail


def snappy_decode(src, cap=None):
    """Snappy raw-format chunk -> bytes. ValueError on anything libsnappy refuses."""
    n, ip, ulen = len(src), 0, 0
    for i in range(6):
        if i == 5:
            raise ValueError("length varint longer than five bytes")
        if ip >= n:
            raise ValueError("input ends in the length")
        b = src[ip]
        ip += 1
        ulen |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            break
    if cap is not None and ulen > cap:
        raise ValueError("announced length larger than the block")
    out = bytearray()
    while ip < n:
        tag = src[ip]
        ip += 1
        if tag & 3 == 0:
            k = tag >> 2
            if k >= 60:
                nb = k - 59
                if ip + nb > n:
                    raise ValueError("input ends in a literal length")
                k = int.from_bytes(src[ip:ip + nb], "little")
                ip += nb
            k += 1
            if ip + k > n:
                raise ValueError("literal runs past the chunk")
            out += src[ip:ip + k]
            ip += k
        else:
            nb = {1: 1, 2: 2, 3: 4}[tag & 3]
            if ip + nb > n:
                raise ValueError("input ends in an offset")
            if tag & 3 == 1:
                length, dist = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | src[ip]
            else:
                length, dist = 1 + (tag >> 2), int.from_bytes(src[ip:ip + nb], "little")
            ip += nb
            _extend(out, dist, length)
        if len(out) > ulen:
            raise ValueError("more output than announced")
    if len(out) != ulen:
        raise ValueError("less output than announced")
    return bytes(out)


def chunk_decode(codec, chunk, cap=None):
    if codec == "lzo":
        return lzo_decode(chunk)
    if codec == "snappy":
        return snappy_decode(chunk, cap)
    return lz4_walk(chunk)[0]


def stream_decode(codec, stream):
    """Hadoop block stream -> (bytes, non-empty blocks), as the device plans it: [u32 BE raw] then
    [u32 BE clen][chunk] until the block's raw bytes are out; an LZO or LZ4 block is one chunk."""
    out, blocks, i, n = bytearray(), 0, 0, len(stream)
    while i < n:
        if i + 4 > n:
            raise ValueError("framing: short block header")
        raw = int.from_bytes(stream[i:i + 4], "big")
        i += 4
        if raw == 0:
            continue
        blocks += 1
        left = raw
        while left > 0:
            if i + 4 > n:
                raise ValueError("framing: short chunk header")
            clen = int.from_bytes(stream[i:i + 4], "big")
            i += 4
            if i + clen > n:
                raise ValueError("framing: chunk longer than the stream")
            got = chunk_decode(codec, stream[i:i + clen], left)
            i += clen
            if len(got) > left or not got or (codec != "snappy" and len(got) != left):
                raise ValueError("block size differs from what was announced")
            out += got
            left -= len(got)
    return bytes(out), blocks


def blocks_of(codec, stream):
    """(announced raw length, [chunks]) per non-empty block of a well-framed stream of valid chunks."""
    i = 0
    while i < len(stream):
        raw = int.from_bytes(stream[i:i + 4], "big")
        i += 4
        if raw == 0:
            continue
        chunks, left = [], raw
        while left > 0:
            clen = int.from_bytes(stream[i:i + 4], "big")
            chunks.append(stream[i + 4:i + 4 + clen])
            i += 4 + clen
            left -= len(snappy_decode(chunks[-1])) if codec == "snappy" else left
        yield raw, chunks


# ------------------------------------------------------------------------------------------- assemblers
class _Asm:
    def __init__(self, seed, base=0):
        self.rng = random.Random(seed)
        self.buf, self.out, self.toks, self.state, self.base = bytearray(), bytearray(), [], 0, base

    @property
    def ip(self):
        return self.base + len(self.buf)

    def _tok(self, kind, size, dist=0, length=0, trail=0):
        self.toks.append(Tok(kind, self.ip, len(self.out), size, self.state, dist, length, trail))

    def _payload(self, n):
        data = self.rng.randbytes(n)
        self.buf += data
        self.out += data

    def _copy(self, dist, length, check):
        assert not check or 1 <= dist <= len(self.out), (dist, len(self.out))
        if 1 <= dist <= len(self.out):
            _extend(self.out, dist, length)

    def near(self, most=48):
        return self.rng.randint(1, min(len(self.out), most))


class Lzo(_Asm):
    @staticmethod
    def lit_header(n):
        if n <= 18:
            return bytes([n - 3])
        k, b = divmod(n - 19, 255)
        return bytes(1 + k) + bytes([b + 1])

    @staticmethod
    def _ext(n):
        k, b = divmod(n - 1, 255)
        return bytes(k) + bytes([b + 1])

    def first(self, n):
        """The first-byte literal run: 1..3 bytes leave state 1..3, 4..238 state 4."""
        assert not self.buf and 1 <= n <= 238
        self._tok("first", 1, length=n)
        self.buf.append(17 + n)
        self._payload(n)
        self.state = n if n < 4 else 4

    def lit(self, n):
        assert self.state == 0 and n >= 4
        h = self.lit_header(n)
        self._tok("lit", len(h), length=n)
        self.buf += h
        self._payload(n)
        self.state = 4

    def match(self, dist, length, trail=0, kind=None, check=True):
        if kind is None:
            kind = ("m1s" if length == 2 else "m2" if length <= 8 and dist <= 2048 else "m3" if dist <= 16384 else "m4")
        assert 0 <= trail <= 3
        if kind in ("m1s", "m1r"):
            if kind == "m1s":
                assert self.state in (1, 2, 3) and length == 2 and 1 <= dist <= 1024
            else:
                assert self.state == 4 and length == 3 and 2049 <= dist <= 3072
            d = dist - (1 if kind == "m1s" else 2049)
            enc = bytes([((d & 3) << 2) | trail, d >> 2])
        elif kind == "m2":
            assert 3 <= length <= 8 and 1 <= dist <= 2048
            enc = bytes([((length - 1) << 5) | (((dist - 1) & 7) << 2) | trail, (dist - 1) >> 3])
        elif kind == "m3":
            assert length >= 3 and 1 <= dist <= 16384
            head = bytes([32 | (length - 2)]) if length <= 33 else bytes([32]) + self._ext(length - 33)
            enc = head + struct.pack("<H", ((dist - 1) << 2) | trail)
        else:
            assert kind == "m4" and length >= 3 and 16385 <= dist <= 49151
            hi, d = divmod(dist - 16384, 16384)
            head = bytes([16 | (hi << 3) | (length - 2)]) if length <= 9 else bytes([16 | (hi << 3)]) + self._ext(length - 9)
            enc = head + struct.pack("<H", (d << 2) | trail)
        self._tok(kind, len(enc), dist, length, trail)
        self.buf += enc
        self._copy(dist, length, check)
        self._payload(trail)
        self.state = trail

    def end(self):
        self._tok("end", 3)
        self.buf += LZO_MARKER

    def lit_to(self, pos):
        """Literal run ending at input offset pos (a 2-byte M2 first where the state or the header sizes ask)."""
        while True:
            if self.state != 0:
                self.match(self.near(), 3, kind="m2")
            rem = pos - self.ip
            assert rem >= 5, rem
            for h in range(1, 12):
                if rem - h >= 4 and len(self.lit_header(rem - h)) == h:
                    return self.lit(rem - h)
            self.match(self.near(), 3, kind="m2")

    def goto(self, target, state, rw):
        """Pad so that the next token starts at input offset `target` in `state`, the register window
        stepping over the multiples of rw on the way (an M2 anchor at each)."""
        a = (self.ip // rw + 1) * rw
        while a <= target - 16:
            if a - self.ip >= 12:
                self.lit_to(a)
                self.match(self.near(), 3, kind="m2")
            a += rw
        self.lit_to(target - (0 if state == 4 else 2 + state))
        if state != 4:
            self.match(self.near(), self.rng.randint(3, 8), state, "m2")
        assert self.ip == target and self.state == state

    def finish(self, more=True):
        if more:
            self.match(self.near(), 4, self.rng.randint(0, 3), "m2")
            if self.state == 0:
                self.lit(self.rng.randint(4, 30))
        self.end()
        return bytes(self.buf), bytes(self.out)


class Snappy(_Asm):
    """Token offsets count from the chunk's start: pass the length of the varint (vlen) up front."""

    def __init__(self, seed, vlen=2):
        super().__init__(seed, vlen)

    def lit(self, n, nbytes=None):
        """nbytes: 0 = length in the tag (1..60), 1..4 = tags 60..63 with that many length bytes."""
        if nbytes is None:
            nbytes = 0 if n <= 60 else ((n - 1).bit_length() + 7) // 8
        assert n >= 1 and (n <= 60 if nbytes == 0 else n - 1 < 1 << (8 * nbytes))
        enc = bytes([(n - 1) << 2]) if nbytes == 0 else bytes([(59 + nbytes) << 2]) + (n - 1).to_bytes(nbytes, "little")
        self._tok("lit" if nbytes == 0 else "lit%d" % (59 + nbytes), len(enc), length=n)
        self.buf += enc
        self._payload(n)

    def copy(self, dist, length, kind=None, check=True):
        if kind is None:
            kind = 1 if 4 <= length <= 11 and dist < 2048 else 2 if dist < 65536 else 4
        if kind == 1:
            assert 4 <= length <= 11 and 0 <= dist < 2048
            enc = bytes([1 | ((length - 4) << 2) | ((dist >> 8) << 5), dist & 255])
        else:
            assert 1 <= length <= 64 and 0 <= dist < 1 << (16 if kind == 2 else 32)
            enc = bytes([(2 if kind == 2 else 3) | ((length - 1) << 2)]) + dist.to_bytes(kind, "little")
        self._tok("copy%d" % kind, len(enc), dist, length)
        self.buf += enc
        self._copy(dist, length, check)

    def lit_to(self, pos):
        rem = pos - self.ip
        for nbytes in range(5):
            n = rem - 1 - nbytes
            if n >= 1 and (n <= 60 if nbytes == 0 else n - 1 < 1 << (8 * nbytes)):
                return self.lit(n, nbytes)
        raise AssertionError(rem)

    def goto(self, target, rw):
        a = (self.ip // rw + 1) * rw
        while a <= target - 16:
            if a - self.ip >= 12:
                self.lit_to(a)
                self.copy(self.near(), 4, 1)
            a += rw
        self.lit_to(target)
        assert self.ip == target

    @staticmethod
    def varint(n, vlen):
        assert n < 1 << (7 * vlen)
        return bytes(((n >> (7 * i)) & 0x7F) | (0x80 if i < vlen - 1 else 0) for i in range(vlen))

    def finish(self, more=True):
        if more:
            self.copy(self.near(), self.rng.randint(1, 64), 2)
            self.lit(self.rng.randint(1, 30))
        return self.varint(len(self.out), self.base) + bytes(self.buf), bytes(self.out)


class Lz4(_Asm):
    @staticmethod
    def _ext(n):
        if n < 15:
            return b""
        k, b = divmod(n - 15, 255)
        return b"\xff" * k + bytes([b])

    def seq(self, nlit, dist, mlen, check=True):
        assert mlen >= 4 and 0 <= dist < 65536
        le, me = self._ext(nlit), self._ext(mlen - 4)
        self._tok("seq", 1 + len(le) + 2 + len(me), dist, mlen, nlit)
        self.buf += bytes([(min(nlit, 15) << 4) | min(mlen - 4, 15)]) + le
        self._payload(nlit)
        self.buf += struct.pack("<H", dist) + me
        self._copy(dist, mlen, check)

    def last(self, nlit):
        le = self._ext(nlit)
        self._tok("last", 1 + len(le), trail=nlit)
        self.buf += bytes([min(nlit, 15) << 4]) + le
        self._payload(nlit)

    def off_to(self, pos):
        """A sequence whose 2-byte offset sits at input offset pos (the next token at pos + 2)."""
        while True:
            rem = pos - self.ip
            assert rem >= 2, rem
            for e in range(0, 12):
                n = rem - 1 - e
                if n >= 1 and len(self._ext(n)) == e:
                    return self.seq(n, self.rng.randint(1, min(len(self.out) + n, 48)), 4)
            self.seq(1, 1, 4)

    def goto(self, target, rw):
        a = (self.ip // rw + 1) * rw
        while a <= target - 16:
            if a - self.ip >= 12:
                self.off_to(a)
            a += rw
        self.off_to(target - 2)
        assert self.ip == target

    def finish(self, more=True):
        if more:
            self.last(self.rng.randint(1, 30))
        return bytes(self.buf), bytes(self.out)


# ------------------------------------------------------------------------------------------ framing
def frame(blocks):
    """blocks: a list of blocks, each a list of (chunk, raw) -> (stream, per-block raws). A block without
    output is framed the way Hadoop frames no data: a zero length and no chunk."""
    stream, braws = bytearray(), []
    for chunks in blocks:
        raw = b"".join(r for _, r in chunks)
        stream += struct.pack(">I", len(raw))
        if not raw:
            continue
        braws.append(raw)
        for c, _ in chunks:
            stream += struct.pack(">I", len(c)) + c
    return bytes(stream), braws


def _case(name, codec, blocks, toks=(), tag=None):
    stream, braws = frame(blocks)
    return Case(name, codec, stream, b"".join(braws), tuple(braws), tuple(toks), tag)


def _one(name, codec, asm, tag=None, more=True):
    chunk, raw = asm.finish(more)
    return _case(name, codec, [[(chunk, raw)]], asm.toks, tag)


def filler(codec, n):
    """A valid one-block stream of exactly n bytes (13..28): what batch() puts between two streams."""
    assert 13 <= n <= 28
    if codec == "lzo":
        a = Lzo(n)
        a.first(n - 12)
    elif codec == "snappy":
        a = Snappy(n, 1)
        a.lit(n - 10)
    else:
        a = Lz4(n)
        if n == 24:  # 15 literals and more take a length byte: no single run makes 24 bytes
            a.seq(1, 1, 4)
            a.last(11)
        else:
            a.last(n - 9 if n < 24 else n - 10)
    c = _one("filler%d" % n, codec, a, more=False)
    assert len(c.stream) == n
    return c


def batch(codec, cases, phase, align):
    """The streams of one launch: every case's stream starts at `phase` modulo `align` of the staged input
    (the first chunk of a stream 8 bytes later), fillers in between. -> (streams, outputs, block raws)."""
    streams, outs, braws, pos = [], [], [], 0
    for c in cases:
        need = (phase - pos) % align
        if need:
            f = filler(codec, need if need >= 13 else need + align)
            streams.append(f.stream)
            outs.append(f.raw)
            braws += f.braws
            pos += len(f.stream)
        streams.append(c.stream)
        outs.append(c.raw)
        braws += c.braws
        pos += len(c.stream)
    return streams, outs, braws


# ------------------------------------------------------------------------------------------ families
def edge_offsets(geom):
    return [(w, x) for w in (geom["reg_window"], 2 * geom["reg_window"], geom["lds_window"]) for x in range(w - 7, w + 5)]


LZO_EDGE_KINDS = ("lit", "lit_ext", "m1s", "m1r", "m2", "m3", "m3_ext", "m4", "m4_hi", "m4_ext", "end")
SNAPPY_EDGE_KINDS = ("lit", "lit60", "lit61", "lit62", "lit63", "copy1", "copy2", "copy4")
LZ4_EDGE_KINDS = ("plain", "lit_ext", "match_ext", "both_ext", "last")
_LZO_MIN_OUT = {"m1s": 1100, "m2": 2100, "m1r": 3100, "m3": 3100, "m3_ext": 3100, "m4": 17000, "m4_hi": 33500,
                "m4_ext": 33500}


def _lzo_start(name, min_out=100):
    """41 random bytes, then a match that repeats them up to min_out bytes of output: state 0."""
    a = Lzo(_seed(name))
    a.first(41)
    a.match(41, max(min_out - 41, 3), kind="m3")
    return a


def _lzo_state_for(kind, rng):
    return 0 if kind in ("lit", "lit_ext") else rng.randint(1, 3) if kind == "m1s" else 4 if kind == "m1r" else rng.randint(0, 4)


def _lzo_emit(a, kind, zeros=2):
    r, n = a.rng, len(a.out)
    trail = r.randint(0, 3)
    if kind == "lit":
        a.lit(r.randint(4, 18))
    elif kind == "lit_ext":
        a.lit(18 + 255 * zeros + r.randint(1, 255))
    elif kind == "m1s":
        a.match(r.randint(1, min(n, 1024)), 2, trail, "m1s")
    elif kind == "m1r":
        a.match(r.randint(2049, 3072), 3, trail, "m1r")
    elif kind == "m2":
        a.match(r.randint(1, min(n, 2048)), r.randint(3, 8), trail, "m2")
    elif kind == "m3":
        a.match(r.randint(1, min(n, 16384)), r.randint(3, 33), trail, "m3")
    elif kind == "m3_ext":
        a.match(r.randint(1, min(n, 16384)), 33 + 255 * zeros + r.randint(1, 255), trail, "m3")
    elif kind == "m4":
        a.match(r.randint(16385, min(n, 32767)), r.randint(3, 9), trail, "m4")
    elif kind == "m4_hi":
        a.match(r.randint(32768, min(n, 49151)), r.randint(3, 9), trail, "m4")
    elif kind == "m4_ext":
        a.match(r.randint(16385, min(n, 49151)), 9 + 255 * zeros + r.randint(1, 255), trail, "m4")
    else:
        assert kind == "end"


def _snappy_start(name, vlen=2):
    a = Snappy(_seed(name), vlen)
    a.lit(41)
    a.copy(41, 60, 2)
    return a


def _snappy_emit(a, kind):
    r, n = a.rng, len(a.out)
    if kind == "lit":
        a.lit(r.randint(1, 60), 0)
    elif kind.startswith("lit"):
        a.lit(r.randint(61, 200), int(kind[3:]) - 59)
    else:
        k = int(kind[4:])
        a.copy(r.randint(1, min(n, 2047)), r.randint(4, 11) if k == 1 else r.randint(1, 64), k)


def _lz4_start(name):
    a = Lz4(_seed(name))
    a.seq(41, 41, 30)
    return a


def _lz4_emit(a, kind):
    r = a.rng
    if kind == "last":
        return a.last(r.randint(0, 40))
    nlit = 15 + 255 + r.randint(0, 254) if kind in ("lit_ext", "both_ext") else r.randint(0, 14)
    mlen = 4 + 15 + 255 + r.randint(0, 254) if kind in ("match_ext", "both_ext") else r.randint(4, 18)
    a.seq(nlit, r.randint(1, len(a.out) + nlit), mlen)


def family_token_at_window_edge(geom):
    rw, out = geom["reg_window"], []
    for w, x in edge_offsets(geom):
        for kind in LZO_EDGE_KINDS:
            name = "edge-lzo-%s-%d-%d" % (kind, w, x)
            a = _lzo_start(name, _LZO_MIN_OUT.get(kind, 100))
            a.goto(x, _lzo_state_for(kind, a.rng), rw)
            _lzo_emit(a, kind)
            out.append(_one(name, "lzo", a, (kind, w, x), more=kind != "end"))
        for kind in SNAPPY_EDGE_KINDS:
            name = "edge-snappy-%s-%d-%d" % (kind, w, x)
            a = _snappy_start(name)
            a.goto(x, rw)
            _snappy_emit(a, kind)
            out.append(_one(name, "snappy", a, (kind, w, x)))
        for kind in LZ4_EDGE_KINDS:
            name = "edge-lz4-%s-%d-%d" % (kind, w, x)
            a = _lz4_start(name)
            a.goto(x, rw)
            _lz4_emit(a, kind)
            out.append(_one(name, "lz4", a, (kind, w, x), more=kind != "last"))
    return out


def family_extension_runs(geom):
    """The byte that ends a zero-run (LZO) or 0xFF-run (LZ4) of 0, 1, 2 and 5 bytes on every edge offset,
    and the lengths on both sides of the first and second extension byte."""
    rw, out = geom["reg_window"], []
    for w, x in edge_offsets(geom):
        for k in RUN_BYTES:
            for kind in ("lit_ext", "m3_ext", "m4_ext"):
                name = "run-lzo-%s-%d-%d-%d" % (kind, k, w, x)
                a = _lzo_start(name, _LZO_MIN_OUT.get(kind, 100) if kind != "m4_ext" else 17000)
                a.goto(x - 1 - k, _lzo_state_for(kind, a.rng), rw)
                _lzo_emit(a, kind, k)
                assert a.buf[x] != 0 and not any(a.buf[x - k:x])
                out.append(_one(name, "lzo", a, (kind, k, w, x)))
            for kind in ("lit_ext", "match_ext"):
                name = "run-lz4-%s-%d-%d-%d" % (kind, k, w, x)
                a = _lz4_start(name)
                a.goto(x - 1 - k - (5 if kind == "match_ext" else 0), rw)
                if kind == "lit_ext":
                    a.seq(15 + 255 * k + a.rng.randint(0, 254), a.near(), 6)
                else:
                    a.seq(3, a.near(), 4 + 15 + 255 * k + a.rng.randint(0, 254))
                assert a.buf[x] != 255 and a.buf[x - k:x] == b"\xff" * k
                out.append(_one(name, "lz4", a, (kind, k, w, x)))
    for n in (18, 19, 273, 274):
        a = _lzo_start("len-lzo-lit-%d" % n)
        a.lit(n)
        out.append(_one("len-lzo-lit-%d" % n, "lzo", a, ("lit_len", n)))
        a = _lz4_start("len-lz4-lit-%d" % n)  # LZ4's own first and second extension byte: 14/15, 269/270
        a.seq(n - 4, a.near(), 4 + n - 4)
        out.append(_one("len-lz4-%d" % n, "lz4", a, ("lit_len", n - 4)))
    for n in (33, 34, 288, 289):
        a = _lzo_start("len-lzo-m3-%d" % n)
        a.match(a.near(), n, a.rng.randint(0, 3), "m3")
        out.append(_one("len-lzo-m3-%d" % n, "lzo", a, ("m3_len", n)))
    for n in (9, 10, 264, 265):
        a = _lzo_start("len-lzo-m4-%d" % n, 17000)
        a.match(16385 + a.rng.randint(0, 500), n, a.rng.randint(0, 3), "m4")
        out.append(_one("len-lzo-m4-%d" % n, "lzo", a, ("m4_len", n)))
    return out


def family_literal_lengths(geom):
    """Every length at source offsets 0..3 (mod reg_align) and destination offsets 0, 1, 15 (mod vec_bytes),
    and literals of up to short_copy bytes that start late in the first register window."""
    ra, vb, sc, rw, out = geom["reg_align"], geom["vec_bytes"], geom["short_copy"], geom["reg_window"], []
    for n in LITERAL_LENGTHS:
        for pi in range(ra):
            for po in (0, 1, vb - 1):
                tag = ("lit", n, pi, po)
                # LZO: first(n0), a 3-byte M3 of length m (1..3 literals ride on it), then the run
                name = "lit-lzo-%d-%d-%d" % tag[1:]
                a = Lzo(_seed(name))
                h = 0 if n < 4 else len(Lzo.lit_header(n))
                n0 = 21 + (pi - (21 + 4 + h)) % ra
                m = 3 + (po - (n0 + 3)) % vb
                a.first(n0)
                a.match(a.near(), m, n if n < 4 else 0, "m3")
                if n >= 4:
                    a.lit(n)
                t = a.toks[-1]  # the run, or the match that carries the literals
                src, dst = t.ip + t.size, t.op + (0 if n >= 4 else t.length)
                assert src % ra == pi and dst % vb == po, (name, src, dst)
                out.append(_one(name, "lzo", a, tag))
                # Snappy: lit(n0), copy2 of length m, the literal
                name = "lit-snappy-%d-%d-%d" % tag[1:]
                a = Snappy(_seed(name), 2)
                h = 1 if n <= 60 else 2 if n <= 256 else 3
                n0 = 21 + (pi - (2 + 1 + 21 + 3 + h)) % ra
                m = 3 + (po - (n0 + 3)) % vb
                a.lit(n0)
                a.copy(a.near(), m, 2)
                a.lit(n)
                t = a.toks[-1]
                assert (t.ip + t.size) % ra == pi and t.op % vb == po, name
                out.append(_one(name, "snappy", a, tag))
                # LZ4: seq(n0 literals, match m), then a sequence with the n literals
                name = "lit-lz4-%d-%d-%d" % tag[1:]
                a = Lz4(_seed(name))
                h = 1 + len(Lz4._ext(n))
                n0 = 5 + (pi - (1 + 5 + 2 + 1 + h)) % ra  # the match length 20..35 has one extension byte
                m = 20 + (po - (n0 + 20)) % vb
                a.seq(n0, a.rng.randint(1, n0), m)
                a.seq(n, a.rng.randint(1, n0), 5)
                t = a.toks[-1]
                assert (t.ip + h) % ra == pi and t.op % vb == po, name
                out.append(_one(name, "lz4", a, tag))
    for s in range(rw - sc - 2, rw):  # 190..255: the refill inside the short literal copy
        tag = ("late_lit", s, sc)
        name = "late-lzo-%d" % s
        a = _lzo_start(name)
        a.goto(s - len(Lzo.lit_header(sc)), 0, rw)
        a.lit(sc)
        out.append(_one(name, "lzo", a, tag))
        name = "late-lz4-%d" % s
        a = _lz4_start(name)
        a.goto(s - 1 - len(Lz4._ext(sc)), rw)
        a.seq(sc, a.near(), 4)
        out.append(_one(name, "lz4", a, tag))
        name = "late-snappy-%d" % s
        a = _snappy_start(name)
        a.goto(s - 2, rw)
        a.lit(sc)
        out.append(_one(name, "snappy", a, tag))
    return out


def _grow(a, codec, dist):
    """601 random bytes, repeated until `dist` bytes are out (601 is prime: no power of two is a period)."""
    base = 601
    if codec == "lzo":
        a.lit(base)
        if dist > base:
            a.match(base, dist - base + a.rng.randint(0, 40), kind="m3")
    elif codec == "lz4":
        a.seq(base, base, max(dist - base, 0) + a.rng.randint(4, 40))
    else:
        a.lit(base)
        while len(a.out) < dist:
            a.copy(base, 64, 2)


def relation(dist, length):
    return "off<len" if dist < length else "off==len" if dist == length else "off>len"


def family_match_shapes(geom):
    out = []
    for dist in MATCH_OFFSETS:
        for length in MATCH_LENGTHS:
            kinds = []
            if length == 2:
                kinds += ["m1s"] if dist <= 1024 else []
            else:
                kinds += ["m2"] if length <= 8 and dist <= 2048 else []
                kinds += ["m1r"] if length == 3 and 2049 <= dist <= 3072 else []
                kinds += ["m3"] if dist <= 16384 else ["m4"]
            for kind in kinds:
                name = "shape-lzo-%s-%d-%d" % (kind, dist, length)
                a = Lzo(_seed(name))
                _grow(a, "lzo", dist)
                if kind == "m1s":
                    a.match(a.near(), 3, a.rng.randint(1, 3), "m2")
                elif kind == "m1r" and a.state != 4:
                    a.lit(5)
                a.match(dist, length, a.rng.randint(0, 3), kind)
                out.append(_one(name, "lzo", a, (kind, dist, length)))
            if length <= 64:
                for k in (1, 2, 4):
                    if k == 1 and not (4 <= length <= 11 and dist < 2048):
                        continue
                    name = "shape-snappy-copy%d-%d-%d" % (k, dist, length)
                    a = Snappy(_seed(name), 3)
                    _grow(a, "snappy", dist)
                    a.copy(dist, length, k)
                    out.append(_one(name, "snappy", a, ("copy%d" % k, dist, length)))
            if length >= 4:
                name = "shape-lz4-%d-%d" % (dist, length)
                a = Lz4(_seed(name))
                _grow(a, "lz4", dist)
                a.seq(a.rng.randint(0, 3), dist, length)
                out.append(_one(name, "lz4", a, ("seq", dist, length)))
    a = Snappy(_seed("shape-snappy-copy4-far"), 3)  # an offset that needs the third offset byte
    _grow(a, "snappy", 70000)
    a.copy(69999, 40, 4)
    out.append(_one("shape-snappy-copy4-69999-40", "snappy", a, ("copy4", 69999, 40)))
    return out


def family_fence(geom):
    """A copy that reads what the copy just before it wrote (and far/near pairs around one), each with both
    copies at most short_copy bytes, both longer, and mixed. One run decides: these can race."""
    sc, out = geom["short_copy"], []
    for codec in CODECS:
        for pat in ("lit_match", "match_match", "far_after_near", "near_after_far"):
            for sizes in ("ss", "ll", "sl", "ls"):
                for rep in range(2):
                    name = "fence-%s-%s-%s-%d" % (codec, pat, sizes, rep)
                    r = random.Random(_seed(name))
                    n1, n2 = (r.randint(8, sc) if c == "s" else r.randint(sc + 1, 5 * sc) for c in sizes)
                    if codec == "snappy":
                        m1, m2 = min(n1, 64), min(n2, 64)
                        a = Snappy(_seed(name), 2)
                        a.lit(2000 if pat != "lit_match" else n1)
                        if pat == "lit_match":
                            a.copy(r.randint(1, n1), m2)
                        elif pat == "match_match":
                            a.copy(r.randint(1, 300), m1)
                            a.copy(r.randint(1, m1), m2)
                        elif pat == "far_after_near":
                            a.copy(r.randint(1, 16), m1)
                            a.copy(r.randint(1500, 1900), m2)
                        else:
                            a.copy(r.randint(1500, 1900), m1)
                            a.copy(r.randint(1, m1), m2)
                    elif codec == "lzo":
                        a = Lzo(_seed(name))
                        a.lit(2000 if pat != "lit_match" else n1)
                        if pat == "lit_match":
                            a.match(r.randint(1, n1), n2, kind="m3")
                        elif pat == "match_match":
                            a.match(r.randint(1, 300), n1, kind="m3")
                            a.match(r.randint(1, n1), n2, kind="m3")
                        elif pat == "far_after_near":
                            a.match(r.randint(1, 16), n1, kind="m3")
                            a.match(r.randint(1500, 1900), n2, kind="m3")
                        else:
                            a.match(r.randint(1500, 1900), n1, kind="m3")
                            a.match(r.randint(1, n1), n2, kind="m3")
                    else:
                        a = Lz4(_seed(name))
                        if pat == "lit_match":
                            a.seq(n1, r.randint(1, n1), n2)
                        else:
                            a.seq(2000, r.randint(1, 300), 8)
                            d1, d2 = {"match_match": (r.randint(1, 300), r.randint(1, n1)),
                                      "far_after_near": (r.randint(1, 16), r.randint(1500, 1900)),
                                      "near_after_far": (r.randint(1500, 1900), r.randint(1, n1))}[pat]
                            a.seq(0, d1, n1)
                            a.seq(0, d2, n2)
                    out.append(_one(name, codec, a, (pat, sizes)))
    return out


def chunk_end_lengths(geom):
    return [n for w in (geom["reg_window"], 2 * geom["reg_window"], geom["lds_window"]) for n in range(w - 3, w + 5)]


def family_chunk_ends(geom):
    """Chunks of exactly 253..260, 509..516 and 2045..2052 bytes that end with a literal, a match or the LZO
    marker: the last register window exactly full, one byte short, one byte over."""
    out = []
    for n in chunk_end_lengths(geom):
        for end in ("lit", "match"):
            name = "end-lzo-%s-%d" % (end, n)
            a = Lzo(_seed(name))
            a.first(30)
            a.match(a.near(), 5, kind="m2")
            if end == "lit":
                a.lit_to(n - 3)
            else:
                t = a.rng.randint(0, 3)
                a.lit_to(n - 3 - 2 - t)
                a.match(a.near(), a.rng.randint(3, 8), t, "m2")
            out.append(_one(name, "lzo", a, (end, n), more=False))
            name = "end-snappy-%s-%d" % (end, n)
            a = Snappy(_seed(name), 2)
            a.lit(30)
            a.copy(a.near(), 9, 1)
            if end == "lit":
                a.lit_to(n)
            else:
                k = a.rng.choice((1, 2, 4))
                a.lit_to(n - 1 - k)
                a.copy(a.near(), a.rng.randint(4, 11), k)
            out.append(_one(name, "snappy", a, (end, n), more=False))
            name = "end-lz4-%s-%d" % (end, n)
            a = Lz4(_seed(name))
            if end == "lit":  # one long final literal run
                a.seq(20, a.rng.randint(1, 20), 9)
                rem = n - a.ip
                k = next(k for k in range(rem - 1, 0, -1) if 1 + len(Lz4._ext(k)) + k == rem)
                a.last(k)
            else:  # a match, then the shortest endings: the lone token 0x00, or a few literals
                k = a.rng.randint(0, 5)
                a.seq(20, a.rng.randint(1, 20), 9)
                a.off_to(n - 1 - k - 2)
                a.last(k)
            out.append(_one(name, "lz4", a, (end, n), more=False))
    for c in out:
        assert int.from_bytes(c.stream[4:8], "big") == c.tag[1] == len(c.stream) - 8, c.name
    # the shortest LZO chunk is the marker alone; it stands for no data, which Hadoop frames as a zero length
    assert lzo_decode(LZO_MARKER) == b""
    out.append(_case("end-lzo-empty", "lzo", [[], []], (), ("empty", 3)))
    return out


LZO_SOUP_KINDS = ("lit", "m1s", "m1r", "m2", "m3", "m4", "end")


def lzo_allowed(state, kind):
    return {"lit": state == 0, "m1s": state in (1, 2, 3), "m1r": state == 4}.get(kind, True)


def family_lzo_states(geom, streams=60, tokens=70):
    """Seeded token soups over every (state, token kind) pair the format allows, every first-byte form, and
    0..3 trailing literals after every match kind."""
    out = []
    for i in range(streams):
        name = "soup-lzo-%d" % i
        a = Lzo(_seed(name))
        r = a.rng
        start = i % 4
        if start == 0:
            a.first(r.randint(1, 3))       # first byte 18..20: state 1..3
        elif start == 1:
            a.first(r.randint(4, 238))     # first byte >= 21: a literal run
        else:
            a.lit(r.randint(4, 400))       # first byte <= 15: the general literal token
        if i % 3 == 0:                     # enough output for M4 distances
            a.match(r.randint(1, len(a.out)), 33000 if i % 2 else 17000, r.randint(0, 3), "m3")
        want_end = i % 5                   # the state the end marker is read in
        for _ in range(tokens):
            n = len(a.out)
            kinds = [k for k in LZO_SOUP_KINDS[:-1] if lzo_allowed(a.state, k)]
            kinds = [k for k in kinds if n >= {"m1r": 2049, "m4": 16385}.get(k, 1)]
            kind = r.choice(kinds)
            trail = r.randint(0, 3)
            if kind == "lit":
                a.lit(r.choice((r.randint(4, 18), r.randint(19, 80), r.randint(81, 600))))
            elif kind == "m1s":
                a.match(r.randint(1, min(n, 1024)), 2, trail, kind)
            elif kind == "m1r":
                a.match(r.randint(2049, min(n, 3072)), 3, trail, kind)
            elif kind == "m2":
                a.match(r.randint(1, min(n, 2048)), r.randint(3, 8), trail, kind)
            elif kind == "m3":
                a.match(r.randint(1, min(n, 16384)), r.choice((r.randint(3, 33), r.randint(34, 400))), trail, kind)
            else:
                a.match(r.randint(16385, min(n, 49151)), r.choice((r.randint(3, 9), r.randint(10, 400))), trail, kind)
        while a.state != want_end:
            if want_end == 4:
                if a.state != 0:
                    a.match(a.near(), 3, 0, "m2")
                a.lit(r.randint(4, 40))
            else:
                a.match(a.near(), r.randint(3, 8), want_end, "m2")
        out.append(_one(name, "lzo", a, ("soup", i), more=False))
    return out


def family_snappy_chunks(geom):
    """Blocks of 1, 2 and 5 chunks with length varints of 1, 2 and 3 bytes; every chunk after the first
    opens with a literal and a copy that reaches back exactly to its own first byte."""
    out = []
    sizes = (100, 1000, 20000, 90, 3000)
    for nchunks in (1, 2, 5):
        for rot in range(3):
            name = "chunks-snappy-%d-%d" % (nchunks, rot)
            chunks, toks = [], []
            for c in range(nchunks):
                want = sizes[(c + rot) % len(sizes)]
                vlen = 1 if want < 128 else 2 if want < 16384 else 3
                a = Snappy(_seed("%s-%d" % (name, c)), vlen)
                k = a.rng.randint(1, 40)
                a.lit(k)
                a.copy(k, a.rng.randint(1, 64), a.rng.choice((2, 4)))
                while len(a.out) < want - 70:
                    if a.rng.random() < 0.4:
                        a.lit(a.rng.randint(1, min(300, want - 64 - len(a.out))))
                    else:
                        a.copy(a.rng.randint(1, len(a.out)), a.rng.randint(1, 64))
                a.lit(a.rng.randint(1, 20))
                chunk, raw = a.finish(False)
                assert max(1, (len(raw).bit_length() + 6) // 7) == vlen, (name, len(raw))
                chunks.append((chunk, raw))
                toks += a.toks
            out.append(_case(name, "snappy", [chunks], toks, (nchunks, rot)))
    return out


def family_layout(geom, pools):
    """The same blocks as 1, 3, 4, 5 and 9 blocks of one stream (idle waves in the last workgroup, mixed
    neighbours), with zero-length blocks in between. pools: codec -> one-block cases to draw from."""
    out = []
    for codec in CODECS:
        pool = pools[codec]
        r = random.Random(_seed("layout-" + codec))
        for k in (1, 3, 4, 5, 9):
            for rep in range(2):
                name = "layout-%s-%d-%d" % (codec, k, rep)
                pick = r.sample(pool, k)
                stream = b"".join((struct.pack(">I", 0) if r.random() < 0.3 else b"") + c.stream for c in pick)
                out.append(Case(name, codec, stream + struct.pack(">I", 0) * rep, b"".join(c.raw for c in pick),
                                tuple(b for c in pick for b in c.braws), (), (k, rep)))
    return out


def family_prefix_targets(geom):
    """Blocks whose prefix decode stops inside a literal or a match of at most short_copy bytes and of more,
    exactly between two tokens, and in a Snappy block's second chunk. tag: (what, the clips to use)."""
    sc, out = geom["short_copy"], []
    for codec in CODECS:
        for what, n1, n2, dist, clips in (
                ("short_literal", sc - 10, 8, 3, (1, 20, sc - 11)),
                ("long_literal", 5 * sc, 8, 3, (sc, sc + 1, 2 * sc + 7, 5 * sc - 1)),
                ("short_match", 10, sc - 4, 10, (11, 30, 10 + sc - 5)),
                ("short_overlapping_match", 10, sc - 4, 3, (11, 30, 10 + sc - 5)),
                ("long_overlapping_match", 7, 4 * sc, 7, (8, sc, sc + 8, 4 * sc)),
                ("long_match", 6 * sc, 4 * sc, 6 * sc - 5, (6 * sc + 1, 7 * sc, 10 * sc - 1)),
                ("token_boundary", 10, 20, 4, (10, 30))):
            name = "clip-%s-%s" % (codec, what)
            if codec == "lzo":
                a = Lzo(_seed(name))
                a.lit(n1)
                a.match(dist, n2, kind="m3")
            elif codec == "snappy":
                a = Snappy(_seed(name), 2)
                a.lit(n1)
                for _ in range(max(n2 // 64, 1)):  # Snappy's longest copy is 64 bytes
                    a.copy(dist, min(n2, 64), 2)
            else:
                a = Lz4(_seed(name))
                a.seq(n1, dist, n2)
            c = _one(name, codec, a, (what, clips))
            out.append(c._replace(tag=(what, clips + (len(c.raw) - 1, len(c.raw), len(c.raw) + 1))))
    chunks = []
    for i, n in enumerate((50, 90)):
        a = Snappy(_seed("clip-snappy-second-chunk-%d" % i), 1)
        a.lit(n - 30)
        a.copy(a.near(), 30, 2)
        chunks.append(a.finish(False))
    out.append(_case("clip-snappy-second-chunk", "snappy", [chunks], (), ("second_chunk", (49, 50, 51, 70, 139, 140))))
    return out


_CACHE = {}


def families(geom):
    """family name -> list of Case, built once per geometry."""
    key = tuple(sorted(geom.items()))
    if key not in _CACHE:
        fam = {
            "token-at-window-edge": family_token_at_window_edge(geom),
            "extension-runs": family_extension_runs(geom),
            "literal-lengths": family_literal_lengths(geom),
            "match-shapes": family_match_shapes(geom),
            "fence": family_fence(geom),
            "chunk-ends": family_chunk_ends(geom),
            "lzo-states": family_lzo_states(geom),
            "snappy-chunks": family_snappy_chunks(geom),
            "prefix-targets": family_prefix_targets(geom),
        }
        pools = {c: [k for f in ("token-at-window-edge", "literal-lengths", "fence", "chunk-ends")
                     for k in fam[f] if k.codec == c and len(k.braws) == 1 and len(k.raw) < 6000] for c in CODECS}
        fam["layout"] = family_layout(geom, pools)
        _CACHE[key] = fam
    return _CACHE[key]


def of_codec(cases, codec):
    return [c for c in cases if c.codec == codec]


# ------------------------------------------------------------------------------------------ corrupt
def _bad(name, codec, chunk, raw_len, whole_chunk=True, stream=None):
    if stream is None:
        stream = struct.pack(">II", raw_len, len(chunk)) + chunk
    return Corrupt(name, codec, stream, chunk if whole_chunk else None, raw_len)


def corrupt_cases(geom):
    """One short named stream per check. Each is refused by a bounds test that the decoders make before the
    access it guards; none is long enough to bring a length near the 32-bit range."""
    out = []

    # ---- LZO1X
    def lzo_with(kind, min_out):
        a = _lzo_start("corrupt-lzo-" + kind, min_out)
        st = _lzo_state_for(kind, a.rng)
        if st == 4:
            a.lit(9)
        elif st:
            a.match(a.near(), 3, st, "m2")
        _lzo_emit(a, kind, 1)
        return a

    for kind in ("lit_ext", "m1s", "m1r", "m2", "m3", "m3_ext", "m4", "m4_ext"):
        a = lzo_with(kind, _LZO_MIN_OUT.get(kind, 100))
        t = a.toks[-1]
        a.finish(False)
        for cut in range(1, t.size):  # the chunk ends after `cut` bytes of the token
            out.append(_bad("lzo-cut-%s-%d" % (kind, cut), "lzo", bytes(a.buf[:t.ip + cut]), len(a.out)))
    a = lzo_with("m2", 100)
    chunk, raw = a.finish(False)
    for cut in (1, 2):
        out.append(_bad("lzo-cut-marker-%d" % cut, "lzo", chunk[:-cut], len(raw)))
    out.append(_bad("lzo-marker-missing", "lzo", chunk[:-3], len(raw)))
    out.append(_bad("lzo-marker-then-a-byte", "lzo", chunk + b"\x00", len(raw)))
    out.append(_bad("lzo-marker-length-4", "lzo", chunk[:-3] + b"\x12\x00\x00", len(raw)))
    out.append(_bad("lzo-marker-extended-length", "lzo", chunk[:-3] + b"\x10\x05\x00\x00", len(raw)))
    out.append(_bad("lzo-output-longer-than-announced", "lzo", chunk, len(raw) - 1, False))
    out.append(_bad("lzo-output-shorter-than-announced", "lzo", chunk, len(raw) + 1, False))
    out.append(_bad("lzo-first-byte-16", "lzo", b"\x10\x01\x00\x00", 40))
    out.append(_bad("lzo-literal-into-last-3-bytes", "lzo", bytes([17 + 10]) + bytes(range(10)) + b"\x11\x00", 10))
    out.append(_bad("lzo-literal-over-the-marker", "lzo", bytes([17 + 13]) + bytes(range(10)) + LZO_MARKER, 13))
    out.append(_bad("lzo-first-literal-past-the-chunk", "lzo", bytes([17 + 200]) + bytes(range(50)), 200))
    for kind, have in (("m1s", 40), ("m2", 40), ("m3", 40), ("m1r", 2500), ("m4", 16390)):
        a = Lzo(_seed("lzo-before-start-" + kind))
        a.first(40)
        if have > 40:
            a.match(40, have - 40 - (5 if kind == "m1r" else 0), kind="m3")
        if kind == "m1s":
            a.match(a.near(), 3, 1, "m2")
        elif kind == "m1r":
            a.lit(5)
        a.match(len(a.out) + 1, 2 if kind == "m1s" else 3, 0, kind, check=False)  # one byte before the output
        a.end()  # room behind the token: the distance test is what refuses
        out.append(_bad("lzo-%s-one-byte-before-the-start" % kind, "lzo", bytes(a.buf), len(a.out) + 3))
    a = Lzo(_seed("lzo-m1r-early"))
    a.first(100)
    a.match(2049, 3, 0, "m1r", check=False)
    a.end()
    out.append(_bad("lzo-m1-after-run-with-100-bytes-out", "lzo", bytes(a.buf), 103))
    first = Lzo(1)
    first.first(30)
    b1 = first.finish(False)
    a = Lzo(2)
    a.first(4)
    a.match(5, 3, 0, "m2", check=False)
    a.end()
    out.append(_bad("lzo-block-2-reaches-into-block-1", "lzo", None, 0, False,
                    frame([[b1]])[0] + struct.pack(">II", 7, len(a.buf)) + bytes(a.buf)))
    a = _lzo_start("lzo-run-to-end", 17000)
    head = bytes(a.buf)
    for side, tok in (("literal", b"\x00"), ("m3", b"\x20"), ("m4", b"\x10")):
        out.append(_bad("lzo-%s-extension-run-to-the-end" % side, "lzo", head + tok + b"\x00" * 300, 200000))

    # ---- Snappy
    for kind in ("lit60", "lit61", "lit62", "lit63", "copy1", "copy2", "copy4"):
        a = _snappy_start("corrupt-snappy-" + kind, 2)
        _snappy_emit(a, kind)
        t = a.toks[-1]
        chunk, raw = a.finish(False)
        for cut in range(1, t.size):
            out.append(_bad("snappy-cut-%s-%d" % (kind, cut), "snappy", chunk[:t.ip + cut], len(raw)))
    a = _snappy_start("corrupt-snappy-ends", 2)
    chunk, raw = a.finish(True)
    out.append(_bad("snappy-literal-past-the-chunk", "snappy", chunk[:-1], len(raw)))
    out.append(_bad("snappy-cut-in-the-length", "snappy", b"\x80", 100))
    out.append(_bad("snappy-chunk-output-longer-than-its-length", "snappy",
                    Snappy.varint(len(raw) - 1, 2) + chunk[2:], len(raw) - 1))
    out.append(_bad("snappy-chunk-output-shorter-than-its-length", "snappy",
                    Snappy.varint(len(raw) + 1, 2) + chunk[2:], len(raw) + 1))
    out.append(_bad("snappy-block-longer-than-announced", "snappy", chunk, len(raw) - 1, False))
    out.append(_bad("snappy-block-shorter-than-announced", "snappy", chunk, len(raw) + 1, False))
    out.append(_bad("snappy-length-of-6-bytes", "snappy", b"\x83\x80\x80\x80\x80\x00" + b"\x08abc", 3))
    out.append(_bad("snappy-length-larger-than-the-block", "snappy", Snappy.varint(1000, 2) + b"\x08abc", 3))
    for k in (1, 2, 4):
        a = Snappy(_seed("snappy-bad-copy%d" % k), 1)
        a.lit(40)
        keep = bytes(a.buf)
        a.copy(0, 5, k, check=False)
        out.append(_bad("snappy-copy%d-offset-0" % k, "snappy", Snappy.varint(45, 1) + bytes(a.buf), 45))
        a.buf[:] = keep
        a.copy(41, 5, k, check=False)
        out.append(_bad("snappy-copy%d-one-byte-before-the-start" % k, "snappy", Snappy.varint(45, 1) + bytes(a.buf), 45))
    a = Snappy(_seed("snappy-copy4-top"), 1)
    a.lit(40)
    a.copy((1 << 24) + 7, 5, 4, check=False)  # only the top offset byte makes it reach too far
    out.append(_bad("snappy-copy4-top-offset-byte", "snappy", Snappy.varint(45, 1) + bytes(a.buf), 45))
    a = Snappy(_seed("snappy-copy4-third"), 1)
    a.lit(40)
    a.copy((1 << 16) + 7, 5, 4, check=False)
    out.append(_bad("snappy-copy4-third-offset-byte", "snappy", Snappy.varint(45, 1) + bytes(a.buf), 45))
    a1 = Snappy(3, 1)
    a1.lit(30)
    c1 = a1.finish(False)
    a2 = Snappy(4, 1)
    a2.lit(4)
    a2.copy(5, 6, 2, check=False)
    c2 = Snappy.varint(10, 1) + bytes(a2.buf)
    out.append(_bad("snappy-chunk-2-reaches-into-chunk-1", "snappy", None, 0, False,
                    struct.pack(">II", 40, len(c1[0])) + c1[0] + struct.pack(">I", len(c2)) + c2))
    out.append(_bad("snappy-block-2-reaches-into-block-1", "snappy", None, 0, False,
                    frame([[c1]])[0] + struct.pack(">II", 10, len(c2)) + c2))
    return out
