"""The device CRC32's state mode (launch_crc32_states, csrc/gpu/crc32.hip): the raw register after a range
from a zero register, no preset and no final inversion, which the host chains over the consecutive slices
of one partition (crc32_fold_state). Oracle: zlib.crc32(seg, 0xFFFFFFFF) ^ 0xFFFFFFFF.
"""
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu
M = 0xFFFFFFFF


def seg_state(seg):
    return zlib.crc32(seg, M) ^ M


@pytest.fixture(scope="module")
def batch(native):
    C = native.gpu_crc32_chunk_bytes()
    rng = random.Random(29)
    # 64C + 5: 65 chunks, so the fold kernel takes more than one 64-chunk group
    lengths = [0, 1, 15, 16, 17, 1023, 1024, 1025, C - 1, C, C + 1, 2 * C + 17, 64 * C + 5]
    items = [rng.randbytes(n) for n in lengths]
    return items, [seg_state(b) for b in items], [zlib.crc32(b) for b in items]  # the references, computed once


@pytest.mark.parametrize("misalign", [0, 1, 15])
def test_states_equal_the_oracle(require_gpu, native, batch, misalign):
    items, want, _ = batch
    got = native.gpu_crc32_states(items, misalign)
    bad = [(len(b), hex(g), hex(w)) for b, g, w in zip(items, got, want) if g != w]
    assert not bad, bad


def test_zero_bytes_have_state_zero(require_gpu, native):
    """A preset leaking into state mode shows here: zeros leave a zero register zero at every length."""
    C = native.gpu_crc32_chunk_bytes()
    items = [bytes(n) for n in (0, 1, 15, 16, 17, 1024, C - 1, C, C + 1, 2 * C + 17)]
    for mis in (0, 15):
        assert native.gpu_crc32_states(items, mis) == [0] * len(items)
    assert native.gpu_crc32_states([]) == []


def test_device_states_folded_on_the_host_give_the_crc_of_the_whole(require_gpu, native):
    C = native.gpu_crc32_chunk_bytes()
    buf = random.Random(31).randbytes(3 * C + 100)
    points = [0, 7, 7, C - 3, 2 * C + 1, len(buf)]
    segs = [buf[a:b] for a, b in zip(points, points[1:])]
    assert b"".join(segs) == buf
    for mis in (0, 1, 15):
        s = M
        for seg, st in zip(segs, native.gpu_crc32_states(segs, mis)):
            s = native.crc32_fold_state(s, st, len(seg))
        assert s ^ M == zlib.crc32(buf)


def test_the_finalized_mode_is_unchanged_over_the_same_batch(require_gpu, native, batch):
    items, _, want = batch
    for mis in (0, 1, 15):
        assert native.gpu_crc32(items, mis) == want
