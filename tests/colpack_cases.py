"""Shared by the colpack tests: the cases, and a pure-numpy implementation of the format
(csrc/codec/colpack.h) that the native host encoder and the device kernels are compared with."""
import struct

import numpy as np

HEADER_BYTES = 640
MAGIC = 0x4B504C43
VERSION = 1
MAX_GROUPS = 32
BUF_RECORDS = (1 << 20) // 104  # records per 1 MiB delivery buffer


def bit_length(v: int) -> int:
    return int(v).bit_length()


def np_encode(recs: np.ndarray, buf_records: int):
    """recs: (n, L) uint8. Returns (piece bytes, packed, S): header alone for a raw piece."""
    n, L = recs.shape
    mn = recs.min(axis=0).astype(np.int64)
    mx = recs.max(axis=0).astype(np.int64)
    width = [bit_length(mx[c] - mn[c]) for c in range(L)]
    G = (L + 7) // 8
    masks, bases, gbs, words = [], [], [], []
    for g in range(G):
        mask = base = 0
        bits = 0
        word = np.zeros(n, np.uint64)
        for c in range(8 * g, min(8 * g + 8, L)):
            k = c - 8 * g
            mask |= ((1 << width[c]) - 1) << (8 * k)
            base |= int(mn[c]) << (8 * k)
            word |= (recs[:, c].astype(np.uint64) - np.uint64(mn[c])) << np.uint64(bits)
            bits += width[c]
        masks.append(mask)
        bases.append(base)
        gbs.append((bits + 7) // 8)
        words.append(word)
    S = sum(gbs)
    packed = not (10 * S > 9 * L)
    pad = MAX_GROUPS - G
    hdr = struct.pack("<IIIIQIII7I", MAGIC, VERSION, L, 1 if packed else 0, n, buf_records, S, G, *([0] * 7))
    hdr += struct.pack(f"<{MAX_GROUPS}Q", *(masks + [0] * pad))
    hdr += struct.pack(f"<{MAX_GROUPS}Q", *(bases + [0] * pad))
    hdr += bytes(gbs + [0] * pad) + bytes(32)
    assert len(hdr) == HEADER_BYTES
    if not packed:
        return hdr, False, S
    rows = np.zeros((n, S), np.uint8)
    off = 0
    for g in range(G):
        for k in range(gbs[g]):
            rows[:, off + k] = ((words[g] >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8)
        off += gbs[g]
    total = (HEADER_BYTES + S * n + 8 + 63) // 64 * 64
    body = rows.tobytes()
    return hdr + body + bytes(total - HEADER_BYTES - len(body)), True, S


def terasort_records(n: int, seed: int) -> np.ndarray:
    """n sorted TeraSort IFile records: [0x0B 0x5B 0x0A] key[10] [0x5A] value[90], values 'A'..'Z'."""
    rng = np.random.RandomState(seed)
    recs = np.zeros((n, 104), np.uint8)
    recs[:, 0:3] = (0x0B, 0x5B, 0x0A)
    hi = np.sort(rng.randint(0, 1 << 62, size=n, dtype=np.int64).astype(np.uint64) << np.uint64(2))
    for b in range(8):
        recs[:, 3 + b] = ((hi >> np.uint64(56 - 8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    recs[:, 11:13] = rng.randint(0, 256, size=(n, 2))
    recs[:, 13] = 0x5A
    recs[:, 14:] = rng.randint(65, 91, size=(n, 90))
    return recs


def _one_column(L: int, n: int, col: int, lo: int, rng_width: int, seed: int) -> np.ndarray:
    """Every column constant except `col`, whose values span exactly [lo, lo + rng_width]."""
    rng = np.random.RandomState(seed)
    recs = np.tile(rng.randint(0, 256, size=(1, L)).astype(np.uint8), (n, 1))
    v = rng.randint(lo, lo + rng_width + 1, size=n)
    v[0], v[-1] = lo, lo + rng_width
    recs[:, col] = v
    return recs


def cases():
    """name -> (records (n, L) uint8, expectation: None, "raw", or the largest stride allowed)."""
    out = {}
    for n in (1, 7, 255, 256, 257, BUF_RECORDS, BUF_RECORDS + 1):
        out[f"terasort_{n}"] = (terasort_records(n, seed=n), 67)
    for r in (0, 1, 127, 128, 255):  # the width boundaries: 0, 1, 7, 8, 8 bits
        out[f"range_{r}"] = (_one_column(104, 300, 21, 0 if r == 255 else 3, r, seed=r), None)
    rng = np.random.RandomState(5)
    wide = np.tile(rng.randint(0, 256, size=(1, 104)).astype(np.uint8), (500, 1))
    wide[:, 40:48] = rng.randint(0, 256, size=(500, 8))  # one group of eight 8-bit columns among width-0 groups
    wide[0, 40:48], wide[1, 40:48] = 0, 255
    out["wide_group"] = (wide, 8)
    out["constant"] = (np.tile(rng.randint(0, 256, size=(1, 104)).astype(np.uint8), (1000, 1)), 0)
    out["random"] = (rng.randint(0, 256, size=(2000, 104)).astype(np.uint8), "raw")
    # tail groups (L % 8 != 0): TeraGen rows without the IFile framing, and records shorter than a group
    out["tail_L100"] = (terasort_records(777, seed=8)[:, 3:103].copy(), None)
    out["tail_L13"] = (rng.randint(60, 70, size=(129, 13)).astype(np.uint8), None)
    out["tail_L5"] = (rng.randint(0, 4, size=(1000, 5)).astype(np.uint8), None)
    out["tail_L255"] = (rng.randint(32, 48, size=(300, 255)).astype(np.uint8), None)
    return out
