"""Hand-assembled zlib (RFC 1950 / 1951) streams for the inflate tests: a bit writer, a fixed-Huffman
assembler and a dynamic-header assembler, and the named valid and invalid cases built with them.

Pure Python and no project code: tests/test_inflate_cases_cpu.py first holds every case against Python's
zlib module (the valid ones decode to `want` with eof set, the invalid ones raise or never reach eof), so
the cases are right by an oracle that is not ours before any of our decoders sees them.
"""
import random
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ZHDR = b"\x78\x9c"
ADLER_TEXT = b"Adler-32 covers the decoded bytes" * 9  # what the adler_mismatch cases decode to


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitlen(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, nbits):
        """A field, least significant bit first."""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """A Huffman code, most significant bit first."""
        self.bits(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def length_symbol(length):
    for i in range(28, -1, -1):
        if length >= LBASE[i] and (i == 28 or length < LBASE[i] + (1 << LEXTRA[i])):
            return 257 + i, LEXTRA[i], length - LBASE[i]
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= DBASE[i]:
            return i, DEXTRA[i], dist - DBASE[i]
    raise ValueError(dist)


def canonical(lens):
    """symbol -> (code, length) of the canonical Huffman code with these lengths."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


class Block:
    """One Huffman block on a BitWriter: fixed code by default, or the code of given lengths."""

    def __init__(self, w, final, lit=None, dist=None):
        self.w = w
        self.lit = lit or FIXED_LIT
        self.dist = dist or FIXED_DIST
        if lit is None:
            w.bits(1 if final else 0, 1)
            w.bits(1, 2)

    def sym(self, s):
        self.w.code(*self.lit[s])

    def lits(self, data):
        for b in data:
            self.sym(b)

    def dsym(self, code):
        self.w.code(*self.dist[code])

    def match(self, length, dist):
        s, eb, ev = length_symbol(length)
        self.sym(s)
        self.w.bits(ev, eb)
        d, eb, ev = dist_symbol(dist)
        self.dsym(d)
        self.w.bits(ev, eb)

    def end(self):
        self.sym(256)


# a complete code-length code without repeats: symbols 0..15 in four bits each
CL_PLAIN = [4] * 16 + [0, 0, 0]
# and one with the repeat symbols: fourteen codes of four bits (0..11, 17, 18), four of five (12, 13, 15, 16)
CL_REPEAT = [4] * 12 + [5, 5, 0, 5, 5, 4, 4]


def dynamic_header(w, final, litlens, distlens, cl_lens=None, cl_syms=None, hlit=None, hdist=None):
    """BTYPE 2 header. cl_syms: the (symbol, extra value) list that codes the lengths; default one symbol
    per length. hlit / hdist override the header's counts (for the invalid cases)."""
    cl_lens = cl_lens or CL_PLAIN
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits((len(litlens) if hlit is None else hlit) - 257, 5)
    w.bits((len(distlens) if hdist is None else hdist) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    if cl_syms is None:
        cl_syms = [(n, 0) for n in list(litlens) + list(distlens)]
    for s, ev in cl_syms:
        w.code(*cl[s])
        if s >= 16:
            w.bits(ev, {16: 2, 17: 3, 18: 7}[s])


def dynamic_block(w, final, litlens, distlens, **kw):
    dynamic_header(w, final, litlens, distlens, **kw)
    return Block(w, final, canonical(litlens), canonical(distlens))


def zwrap(deflate, want, header=ZHDR):
    return header + deflate + zlib.adler32(want).to_bytes(4, "big")


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


def _lit_lens_deep():
    """Literal/length lengths using every length 1..15 (and 15 twice: a complete code). EOB gets one bit so
    the 15-bit codes are literals; symbols: 256 -> 1 bit, 'a'.. -> 2..15 bits."""
    lens = [0] * 286
    lens[256] = 1
    for i, n in enumerate(range(2, 16)):
        lens[ord("a") + i] = n
    lens[ord("z")] = 15
    return lens


def valid_cases(window=256, stage=64):
    """[(name, stream, want)]. window: the device decoder's input window in bytes, stage: its literal staging
    width; the boundary sweeps (boundary_cases) are laid around multiples of them."""
    cases = []

    def add(name, w, want, header=ZHDR):
        cases.append((name, zwrap(w.done(), want, header), want))

    # a match at distance 32768, which zlib's own encoder never emits, of the longest length
    w = BitWriter()
    b = Block(w, True)
    head = _rand(32768, 1)
    b.lits(head)
    b.match(258, 32768)
    b.end()
    add("dist_32768_len_258", w, head + head[:258])

    w = BitWriter()
    b = Block(w, True)
    b.lits(b"a")
    b.match(258, 1)
    b.end()
    add("len_258_dist_1", w, b"a" * 259)

    for d in (1, 2, 3):  # the source is literals that were not stored yet
        w = BitWriter()
        b = Block(w, True)
        b.lits(b"xyz")
        b.match(10, d)
        b.lits(b"!")
        b.end()
        want = bytearray(b"xyz")
        for _ in range(10):
            want.append(want[-d])
        add("pending_literals_dist_%d" % d, w, bytes(want) + b"!")

    w = BitWriter()
    b = Block(w, True)
    b.lits(b"hello")
    b.match(5, 5)  # source starts at output byte 0
    b.lits(b"..")
    b.end()
    add("match_source_at_byte_0", w, b"hellohello..")

    w = BitWriter()
    b = Block(w, True)
    b.lits(b"tail-")
    b.match(4, 5)  # the stream's last byte is the match's last
    b.end()
    add("match_ends_at_last_byte", w, b"tail-tail")

    for n in (stage - 1, stage, stage + 1, 2 * stage - 1, 2 * stage, 2 * stage + 1):
        w = BitWriter()
        b = Block(w, True)
        lit = _rand(n, n)
        b.lits(lit)
        b.match(20, n)
        b.lits(b"end")
        b.end()
        add("literals_%d_then_match" % n, w, lit + (lit * 20)[:20] + b"end")

    w = BitWriter()
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    w.raw(b"\x00\x00\xff\xff")
    add("stored_0", w, b"")

    w = BitWriter()
    big = _rand(65535, 7)
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    w.raw(b"\xff\xff\x00\x00" + big)
    add("stored_65535", w, big)

    # a block that ends at each of the eight bit phases (j nine-bit literals shift it), followed by a
    # stored block / by the stream's end
    for j in range(8):
        lit = b"ab" + bytes([200 + k for k in range(j)])
        w = BitWriter()
        b = Block(w, False)
        b.lits(lit)
        b.end()
        phase = w.bitlen % 8
        w.bits(1, 1)
        w.bits(0, 2)
        w.align()
        body = _rand(100 + j, 40 + j)
        w.raw(len(body).to_bytes(2, "little") + (len(body) ^ 0xFFFF).to_bytes(2, "little") + body)
        add("stored_entered_at_phase_%d" % phase, w, lit + body)
        w = BitWriter()
        b = Block(w, True)
        b.lits(lit)
        b.end()
        add("end_of_block_at_phase_%d" % (w.bitlen % 8), w, lit)

    # sync-flushed raw-deflate segments of three compressors under one header
    text = b"".join(b"%d bottles of beer on the wall, " % (i % 37) for i in range(3000))
    parts, segs = [text[:20000], text[20000:50000], text[50000:]], []
    for i, (level, strategy) in enumerate(((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY))):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        segs.append(c.compress(parts[i]) + c.flush(zlib.Z_FINISH if i == 2 else zlib.Z_SYNC_FLUSH))
    cases.append(("sync_flushed_segments", zwrap(b"".join(segs), text), text))

    # a dynamic block with a single distance code (an incomplete code zlib allows)
    w = BitWriter()
    lens = [0] * 258
    lens[ord("q")] = 1
    lens[256] = 2
    lens[257] = 2  # length 3
    b = dynamic_block(w, True, lens, [1])
    b.lits(b"q")
    b.match(3, 1)
    b.lits(b"q")
    b.match(3, 1)
    b.end()
    add("dynamic_single_distance_code", w, b"q" * 8)

    # a dynamic block using 15-bit codes
    w = BitWriter()
    lens = _lit_lens_deep()
    b = dynamic_block(w, True, lens, [1, 1])
    text15 = b"az" + bytes([ord("a") + 13]) * 3 + b"zzab"
    b.lits(text15)
    b.end()
    add("dynamic_15_bit_codes", w, text15)

    # dynamic header coded with the repeat symbols 16, 17, 18
    w = BitWriter()
    lens = [0] * 97 + [2, 2, 2] + [0] * 156 + [2]  # 'a','b','c' and EOB: four codes of two bits
    syms = [(18, 97 - 11), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (17, 10 - 3), (17, 8 - 3), (2, 0), (0, 0), (16, 0)]
    # (100 + 138 + 10 + 8 = 256 lengths, then EOB's, then distance lengths 0 and three repeats of it: 4 of them)
    dynamic_header(w, True, lens, [0, 0, 0, 0], cl_lens=CL_REPEAT, cl_syms=syms)
    b = Block(w, True, canonical(lens), {})
    b.lits(b"abcabccba")
    b.end()
    add("dynamic_repeat_codes", w, b"abcabccba")

    cases += [c[:3] for c in boundary_cases(window)]
    return cases


def _pad_to(b, w, target):
    """Literals on block b so that the writer's next bit is deflate bit `target`, to the bit: one-byte codes
    (symbols below 144), and target mod 8 of the nine-bit ones to shift the phase. Returns the literals."""
    need = target - w.bitlen
    j = need % 8
    a = (need - 9 * j) // 8
    assert a >= 0 and 8 * a + 9 * j == need
    rng = random.Random(target)
    lit = bytes(rng.randrange(144, 256) for _ in range(j)) + bytes(rng.randrange(144) for _ in range(a))
    b.lits(lit)
    assert w.bitlen == target
    return lit


BOUNDARY_FAMILIES = ("code_straddles_refill", "stored_len_straddles_refill", "dynamic_header_straddles_refill")


def boundary_starts(window, m):
    """Stream bit positions (zlib header included) an item is started at around the m-th window boundary:
    every bit from 8 bytes before it, where the 64-bit bit buffer takes the refill that crosses it, to 2 bytes
    behind it."""
    return range(8 * (m * window - 8), 8 * (m * window + 2) + 1)


def boundary_cases(window=256):
    """[(name, stream, want, family, m, first_bit, last_bit)]: an item laid, to the bit, at every position of
    boundary_starts() around the first two refills of the device decoder's input window (stream bytes
    m * window), behind literal padding. first_bit / last_bit are the item's first bit and the bit behind
    its last one in the stream, zlib header included, so a test can see that the boundary is really crossed.
      code:    a length code with 5 extra bits and a distance code with 6 or 7 (25 bits or so);
      stored:  a stored block's header, first_bit, and its LEN / NLEN field, whose end is last_bit;
      dynamic: a dynamic block's header (153 bytes); started, besides, every 8 bytes from 152 to 16 bytes
               before the boundary, so that the boundary falls in every part of it."""
    out = []
    hdr = 8 * len(ZHDR)
    text15 = b"az" + bytes([ord("a") + 13]) * 3 + b"zzab"
    for m in (1, 2):
        for t in boundary_starts(window, m):
            w = BitWriter()
            b = Block(w, True)
            lit = _pad_to(b, w, t - hdr)
            n = len(lit)
            b.match(200, n)
            last = w.bitlen + hdr
            b.lits(b"Z")
            b.end()
            want = bytearray(lit)
            for _ in range(200):
                want.append(want[-n])
            out.append(("%s_m%d_bit_%d" % (BOUNDARY_FAMILIES[0], m, t), zwrap(w.done(), bytes(want) + b"Z"),
                        bytes(want) + b"Z", BOUNDARY_FAMILIES[0], m, t, last))

            w = BitWriter()
            b = Block(w, False)
            lit = _pad_to(b, w, t - hdr - 7)
            b.end()
            assert w.bitlen + hdr == t
            w.bits(1, 1)
            w.bits(0, 2)
            w.align()
            body = _rand(300, t)
            w.raw(len(body).to_bytes(2, "little") + (len(body) ^ 0xFFFF).to_bytes(2, "little"))
            last = w.bitlen + hdr
            w.raw(body)
            out.append(("%s_m%d_bit_%d" % (BOUNDARY_FAMILIES[1], m, t), zwrap(w.done(), lit + body), lit + body,
                        BOUNDARY_FAMILIES[1], m, t, last))
        early = [8 * (m * window - d) for d in range(152, 8, -8)]
        for t in list(boundary_starts(window, m)) + early:
            w = BitWriter()
            b = Block(w, False)
            lit = _pad_to(b, w, t - hdr - 7)
            b.end()
            lens = _lit_lens_deep()
            dynamic_header(w, True, lens, [1, 1])
            last = w.bitlen + hdr
            b = Block(w, True, canonical(lens), canonical([1, 1]))
            b.lits(text15)
            b.end()
            out.append(("%s_m%d_bit_%d" % (BOUNDARY_FAMILIES[2], m, t), zwrap(w.done(), lit + text15), lit + text15,
                        BOUNDARY_FAMILIES[2], m, t, last))
    return out


def invalid_cases():
    """[(name, stream)]: every stream is refused by zlib's inflate, or never reaches its end."""
    cases = []
    body = zlib.compress(b"hello hello hello hello", 9)[2:]  # deflate + Adler-32 of a valid stream

    cases.append(("header_cm_not_8", b"\x79\x18" + body))         # 0x7918 % 31 == 0, CM = 9
    cases.append(("header_cinfo_8", b"\x88\x1c" + body))          # 0x881c % 31 == 0, CINFO = 8
    cases.append(("header_check", b"\x78\x9d" + body))
    cases.append(("header_fdict", b"\x78\x20" + body))            # 0x7820 % 31 == 0, FDICT set
    assert 0x7918 % 31 == 0 and 0x881c % 31 == 0 and 0x7820 % 31 == 0

    def add(name, w, want=b""):
        cases.append((name, zwrap(w.done(), want)))

    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    add("btype_3", w)

    w = BitWriter()
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    w.raw(b"\x03\x00\xfc\xfe" + b"abc")
    add("stored_len_nlen", w, b"abc")

    ok_lit = [0] * 97 + [2, 2, 2] + [0] * 156 + [2] + [0]  # 258 lengths: 'a','b','c', EOB; 257 none
    for name, hl, hd in (("hlit_287", 287, None), ("hlit_288", 288, None), ("hdist_31", None, 31), ("hdist_32", None, 32)):
        w = BitWriter()
        dynamic_header(w, True, ok_lit, [1, 1], hlit=hl, hdist=hd)
        w.bits(0, 32)
        add(name, w)

    def dyn(name, litlens, distlens, **kw):
        w = BitWriter()
        dynamic_header(w, True, litlens, distlens, **kw)
        w.bits(0, 64)  # something behind the header, so that it is no truncation
        add(name, w)

    over = list(ok_lit)
    over[ord("d")] = 1  # 1/2 + 4/4 > 1
    dyn("oversubscribed_literal_lengths", over, [1, 1])
    dyn("oversubscribed_distance_lengths", ok_lit, [1, 1, 1])
    dyn("oversubscribed_code_length_code", ok_lit, [1, 1], cl_lens=[4] * 16 + [4, 0, 0])
    incomplete = list(ok_lit)
    incomplete[ord("c")] = 0
    dyn("incomplete_literal_lengths", incomplete, [1, 1])
    dyn("incomplete_distance_lengths", ok_lit, [2, 2])
    dyn("incomplete_distance_single_2_bit_code", ok_lit, [2])
    dyn("incomplete_code_length_code", ok_lit, [1, 1], cl_lens=[4] * 15 + [0, 0, 0, 0],
        cl_syms=[(n, 0) for n in ok_lit + [1, 1]])
    dyn("repeat_16_with_no_previous_length", ok_lit, [1, 1], cl_lens=CL_REPEAT, cl_syms=[(16, 0)] + [(0, 0)] * 300)
    # 258 + 2 lengths: 97 zeros, three 2s, 138 zeros, then a run of 30 zeros where 22 are left
    dyn("repeat_past_the_last_length", ok_lit, [1, 1], cl_lens=CL_REPEAT,
        cl_syms=[(18, 97 - 11), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (18, 30 - 11)])
    no_eob = [0] * 97 + [1, 1] + [0] * 159
    dyn("no_code_for_end_of_block", no_eob, [1, 1])

    for s in (286, 287):
        w = BitWriter()
        b = Block(w, True)
        b.lits(b"ab")
        b.sym(s)
        w.bits(0, 24)
        add("fixed_literal_length_symbol_%d" % s, w, b"ab")
    for d in (30, 31):
        w = BitWriter()
        b = Block(w, True)
        b.lits(b"abcdef")
        b.sym(257)
        b.dsym(d)
        w.bits(0, 24)
        add("fixed_distance_code_%d" % d, w, b"abcdef")

    w = BitWriter()
    b = Block(w, True)
    b.lits(b"a")
    b.match(3, 2)
    b.end()
    add("distance_beyond_output", w, b"aaaa")
    w = BitWriter()
    b = Block(w, True)
    b.match(3, 1)  # nothing produced yet
    b.end()
    add("distance_beyond_output_at_start", w, b"")

    good = zlib.compress(ADLER_TEXT, 6)
    cases.append(("adler_mismatch", good[:-1] + bytes([good[-1] ^ 1])))
    cases.append(("adler_mismatch_high_byte", good[:-4] + bytes([good[-4] ^ 0x80]) + good[-3:]))

    # ---- truncation
    text = b"".join(b"%d green bottles hanging on the wall, " % (i * 7919 % 101) for i in range(400))
    dynz = zlib.compress(text, 9)
    assert (dynz[2] >> 1) & 3 == 2  # a dynamic block first
    cases.append(("cut_inside_header", dynz[:1]))
    cases.append(("cut_after_header", dynz[:2]))
    cases.append(("cut_inside_dynamic_header", dynz[:12]))
    cases.append(("cut_inside_symbols", dynz[:len(dynz) // 2]))
    cases.append(("cut_before_adler", dynz[:-4]))
    cases.append(("cut_inside_adler", dynz[:-2]))
    cases.append(("cut_last_byte", dynz[:-1]))
    cases.append(("empty", b""))
    w = BitWriter()
    b = Block(w, True)
    lit = _rand(30000, 5)
    b.lits(lit)
    s, eb, ev = length_symbol(3)
    b.sym(s)
    d, eb, ev = dist_symbol(30000)
    b.dsym(d)
    cut = (w.bitlen + 5) // 8  # the byte that holds the middle of the 13 extra bits is missing
    w.bits(ev, eb)
    b.end()
    whole = zwrap(w.done(), lit + lit[:3])
    cases.append(("cut_inside_extra_bits", whole[:2 + cut]))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    w.raw(b"\x0a\x00\xf5\xff" + b"0123456789")
    whole = zwrap(w.done(), b"0123456789")
    cases.append(("cut_inside_stored_len", whole[:2 + 3]))
    cases.append(("cut_inside_stored_bytes", whole[:2 + 5 + 4]))
    return cases
