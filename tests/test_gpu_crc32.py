"""The device CRC32 (csrc/gpu/crc32.hip) against zlib.crc32: one batched launch over ranges of every
length at which the kernel takes another path (head and tail bytes, partial rows, chunk boundaries), at
every kind of misalignment, with many ranges per launch, and with single flipped bits.
"""
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(native):
    C = native.gpu_crc32_chunk_bytes()
    rng = random.Random(17)
    lengths = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, C - 1, C, C + 1, 2 * C + 7, 3 * C + 1029]
    items = [rng.randbytes(n) for n in lengths]
    for n in (1, 64, C, C + 1):  # zeros catch a wrong length shift, ones the preset
        items += [rng.randbytes(n), bytes(n), b"\xff" * n]
    items.append(b"123456789")
    return items, [zlib.crc32(b) for b in items]  # the reference, computed once


def test_check_value(require_gpu, native):
    assert native.gpu_crc32([b"123456789"]) == [0xCBF43926]
    assert native.gpu_crc32([]) == []
    assert native.gpu_crc32([b""]) == [0]


@pytest.mark.parametrize("misalign", [0, 1, 7, 8, 15])
def test_batch_equals_zlib(require_gpu, native, batch, misalign):
    items, want = batch
    got = native.gpu_crc32(items, misalign)
    bad = [(len(b), hex(g), hex(w)) for b, g, w in zip(items, got, want) if g != w]
    assert not bad, bad


def test_many_small_ranges_around_a_large_one(require_gpu, native):
    """A wrong chunk-to-range mapping or fold order shows when ranges without chunks, with one chunk and
    with several sit in one launch."""
    C = native.gpu_crc32_chunk_bytes()
    rng = random.Random(19)
    items = [rng.randbytes(rng.randint(0, 300)) for _ in range(200)]
    items[100] = rng.randbytes(3 * C + 1)
    for mis in (0, 5):
        assert native.gpu_crc32(items, mis) == [zlib.crc32(b) for b in items]


def test_single_bit_flips_change_the_crc_to_the_flipped_buffers_own(require_gpu, native):
    C = native.gpu_crc32_chunk_bytes()
    base = random.Random(23).randbytes(2 * C)
    items = [base]
    for pos in (0, C - 1, C, 2 * C - 1):
        b = bytearray(base)
        b[pos] ^= 0x04
        items.append(bytes(b))
    want = [zlib.crc32(b) for b in items]
    assert len(set(want)) == len(want)
    for mis in (0, 9):  # at 9 the chunk boundary falls elsewhere in the buffer
        assert native.gpu_crc32(items, mis) == want
