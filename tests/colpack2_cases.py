"""Shared by the colpack version 2 tests: the cases, and an independent numpy / Python-int
implementation of the format (csrc/codec/colpack.h: key differences, restart table, bit-contiguous
rows) that the native host encoder and the device kernels are compared with."""
import functools
import struct

import numpy as np

from tests.colpack_cases import terasort_records

HEADER_BYTES = 640
MAGIC = 0x4B504C43
MAX_GROUPS = 32
FLAG_PACKED, FLAG_DELTA = 1, 2


def key_deltas(recs: np.ndarray, buf_records: int, key_off: int, key_len: int) -> np.ndarray:
    """(n, key_len) uint8: T(r) big-endian; 0 on every buf_records-th row, else K(r) - K(r-1) mod 2^(8 key_len)."""
    n = recs.shape[0]
    keys = [int.from_bytes(recs[r, key_off:key_off + key_len].tobytes(), "big") for r in range(n)]
    mod = 1 << (8 * key_len)
    out = np.zeros((n, key_len), np.uint8)
    for r in range(n):
        t = 0 if r % buf_records == 0 else (keys[r] - keys[r - 1]) % mod
        out[r] = np.frombuffer(t.to_bytes(key_len, "big"), np.uint8)
    return out


def widths(cols: np.ndarray):
    mn = cols.min(axis=0).astype(np.int64)
    mx = cols.max(axis=0).astype(np.int64)
    return mn, [int(mx[c] - mn[c]).bit_length() for c in range(cols.shape[1])]


def layout(group_bits):
    """Bit offset of every group's word and the stride, by the bit-cursor rule."""
    bo, offs = 0, []
    for bits in group_bits:
        if bits and (bo & 7) + bits > 64:
            bo = (bo + 7) // 8 * 8
        offs.append(bo)
        bo += bits
    return offs, (bo + 7) // 8


def np_encode2(recs: np.ndarray, buf_records: int, key_off: int, key_len: int):
    """recs: (n, L) uint8. Returns (piece bytes, packed, delta, S, group bit offsets, group bits)."""
    n, L = recs.shape
    if key_len == 0 or buf_records < 1:
        key_off = key_len = 0
    cols = recs.copy()
    delta = False
    if key_len:
        d = key_deltas(recs, buf_records, key_off, key_len)
        plain_bits = sum(widths(recs[:, key_off:key_off + key_len])[1])
        delta_bits = sum(widths(d)[1])
        entries = (n + buf_records - 1) // buf_records
        delta = delta_bits * n + 128 * entries < plain_bits * n
        if delta:
            cols[:, key_off:key_off + key_len] = d
    mn, width = widths(cols)
    G = (L + 7) // 8
    masks, bases, gbits, words = [], [], [], []
    for g in range(G):
        mask = base = word = 0
        bits = 0
        word = [0] * n
        for c in range(8 * g, min(8 * g + 8, L)):
            k = c - 8 * g
            mask |= ((1 << width[c]) - 1) << (8 * k)
            base |= int(mn[c]) << (8 * k)
            v = cols[:, c].astype(np.int64) - mn[c]
            word = [w | (int(x) << bits) for w, x in zip(word, v)]
            bits += width[c]
        masks.append(mask)
        bases.append(base)
        gbits.append(bits)
        words.append(word)
    offs, S = layout(gbits)
    packed = not (10 * S > 9 * L)
    flags = (FLAG_PACKED if packed else 0) | (FLAG_DELTA if delta else 0)
    pad = MAX_GROUPS - G
    hdr = struct.pack("<IIIIQIIIII5I", MAGIC, 2, L, flags, n, buf_records, S, G, key_off, key_len, *([0] * 5))
    hdr += struct.pack(f"<{MAX_GROUPS}Q", *(masks + [0] * pad))
    hdr += struct.pack(f"<{MAX_GROUPS}Q", *(bases + [0] * pad))
    hdr += struct.pack(f"<{MAX_GROUPS}H", *(offs + [0] * pad))
    assert len(hdr) == HEADER_BYTES
    if not packed:
        return hdr, False, delta, S, offs, gbits
    table = b""
    if delta:
        for b in range(0, n, buf_records):
            table += recs[b, key_off:key_off + key_len].tobytes() + bytes(16 - key_len)
        table += bytes(-len(table) % 64)
    body = bytearray()
    for r in range(n):
        row = 0
        for g in range(G):
            row |= words[g][r] << offs[g]
        body += row.to_bytes(S, "little")
    total = (HEADER_BYTES + len(table) + S * n + 8 + 63) // 64 * 64
    piece = hdr + table + bytes(body)
    return piece + bytes(total - len(piece)), True, delta, S, offs, gbits


def _narrow(n, L, seed, lo=0, hi=2):
    return np.random.RandomState(seed).randint(lo, hi, size=(n, L)).astype(np.uint8)


def _sorted_keys(recs, key_off, key_len, seed, spread_bits):
    """Overwrite the key field with ascending keys whose steps stay below 2^spread_bits."""
    rng = np.random.RandomState(seed)
    k = 0
    for r in range(recs.shape[0]):
        k += int(rng.randint(0, 1 << min(spread_bits, 30))) << max(0, spread_bits - 30)
        recs[r, key_off:key_off + key_len] = np.frombuffer((k % (1 << (8 * key_len))).to_bytes(key_len, "big"), np.uint8)
    return recs


def _bits_case(n, group_bits, seed):
    """Records of 8 * len(group_bits) bytes whose group g has exactly group_bits[g] bits: columns of
    width 8 first, then one of the remainder, every column reaching both ends of its range."""
    rng = np.random.RandomState(seed)
    L = 8 * len(group_bits)
    recs = np.full((n, L), 7, np.uint8)
    for g, bits in enumerate(group_bits):
        for c in range(8):
            w = min(8, bits - 8 * c)
            if w <= 0:
                break
            hi = (1 << w) - 1
            recs[:, 8 * g + c] = rng.randint(0, hi + 1, size=n)
            recs[0, 8 * g + c], recs[n - 1, 8 * g + c] = 0, hi
    return recs


def cases():
    """name -> dict(recs, buf, ko, kl, expect): expect has 'delta' (bool or None), 'packed' (bool or None)."""
    out = {}

    def add(name, recs, buf, ko, kl, delta=None, packed=True):
        out[name] = dict(recs=np.ascontiguousarray(recs), buf=buf, ko=ko, kl=kl, delta=delta, packed=packed)

    tera = terasort_records(2520, seed=11)
    add("terasort_sorted", tera, 78, 3, 10, delta=True)
    rng = np.random.RandomState(12)
    add("terasort_shuffled", tera[rng.permutation(2520)], 78, 3, 10, delta=False, packed=None)
    dup = tera.copy()
    dup[:, 3:13] = dup[(np.arange(2520) // 5) * 5, 3:13]  # runs of five equal keys
    add("duplicate_keys", dup, 78, 3, 10, delta=True)
    # the key crosses the boundary of groups 0 and 1 (and 1 and 2); the key ends at the record's last byte
    add("key_crosses_groups", _sorted_keys(_narrow(600, 40, 13), 5, 12, 13, 40), 50, 5, 12, delta=True)
    add("key_at_record_end", _sorted_keys(_narrow(600, 27, 14), 19, 8, 14, 24), 50, 19, 8, delta=True)
    add("key_len_16_at_0", _sorted_keys(_narrow(500, 24, 15), 0, 16, 15, 70), 64, 0, 16, delta=True)
    add("key_len_0", tera[:300], 78, 0, 0, delta=False)
    add("L_not_multiple_of_8", _sorted_keys(_narrow(333, 21, 16, 0, 8), 2, 6, 16, 20), 40, 2, 6, delta=True)
    # group 0: 5 bits, so group 1 starts at bit 5: 59 bits end exactly at bit 64, 60 bits must be realigned
    add("fits_64_exactly", _bits_case(300, [5, 59, 9], 17), 64, 0, 0, delta=False)
    add("realigned_at_65", _bits_case(300, [5, 60, 9], 18), 64, 0, 0, delta=False)
    # a 64-bit group after a misaligned one, among narrow groups that keep the piece packed
    add("group_64_after_misaligned", _bits_case(300, [3, 64, 2, 1, 0, 0, 0, 0, 0, 0], 19), 64, 0, 0, delta=False)
    add("nrec_1", tera[:1], 78, 3, 10, delta=False)
    add("nrec_not_multiple_of_buf", tera[:2520 - 41], 78, 3, 10, delta=True)
    add("buf_records_1", tera[:400], 1, 3, 10, delta=False)  # the table costs more than the key
    add("all_constant", np.tile(tera[:1], (500, 1)), 78, 3, 10, delta=False)
    add("raw", rng.randint(0, 256, size=(700, 104)).astype(np.uint8), 78, 3, 10, delta=None, packed=False)
    return out


CASES = cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """np_encode2 of a case, computed once and shared by the CPU and the GPU tests."""
    c = CASES[name]
    return np_encode2(c["recs"], c["buf"], c["ko"], c["kl"])
