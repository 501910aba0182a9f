"""Device Adler-32 (csrc/gpu/adler32.hip) against zlib.adler32: one batched launch per misalignment over
lengths around every edge of the sums: none, one byte, 5552 (the most bytes zlib sums before it reduces),
65521 (the modulus) and 65536, and 300000 bytes of 0xFF, the largest sums a range of that size can reach.
"""
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 5551, 5552, 5553, 65520, 65521, 65522, 65535, 65536, 65537]


@pytest.fixture(scope="module")
def items():
    rng = random.Random(32)
    out = [rng.randbytes(n) for n in LENGTHS]
    out += [b"\xff" * n for n in (5552, 65521, 65537)]
    out.append(b"\xff" * 300_000)
    out.append(rng.randbytes(300_000))
    return out


@pytest.fixture(scope="module")
def want(items):
    return [zlib.adler32(it) for it in items]


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_adler32_batched(require_gpu, native, items, want, misalign):
    got = native.gpu_adler32(items, misalign)
    for it, g, w in zip(items, got, want):
        assert g == w, (len(it), it[:1], hex(g), hex(w))


def test_adler32_no_items(require_gpu, native):
    assert native.gpu_adler32([], 0) == []
