"""colpack version 2 device kernels (csrc/gpu/colpack.hip: stats, plan, pack) on small device arrays:
the bytes they write, header, restart table and padding included, equal the host encoder's byte for
byte (which tests/test_colpack2_cpu.py compares with the numpy implementation), and host-decoding them
gives back the input. Same cases as the CPU test, one launch per record length and key setting with
pieces of different sizes."""
import numpy as np
import pytest

from tests.colpack2_cases import CASES, HEADER_BYTES, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_pieces(require_gpu, native):
    """name -> (piece bytes, packed, stride). A launch has one record length, buffer size and key field."""
    by_launch = {}
    for name, c in CASES.items():
        by_launch.setdefault((c["recs"].shape[1], c["buf"], c["ko"], c["kl"]), []).append(name)
    out = {}
    for (L, buf, ko, kl), names in by_launch.items():
        res = native.gpu_colpack2_encode([CASES[n]["recs"].tobytes() for n in names], L, buf, ko, kl)
        out.update(zip(names, res))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_device_pack2_equals_host_encoder(native, device_pieces, name):
    c = CASES[name]
    recs = c["recs"]
    n, L = recs.shape
    piece, packed, stride = device_pieces[name]
    want = native.colpack2_encode(recs.tobytes(), L, c["buf"], c["ko"], c["kl"])
    ref, ref_packed, _, ref_stride, _, _ = reference(name)
    assert want == ref
    assert piece[:HEADER_BYTES] == want[:HEADER_BYTES]
    assert piece == want
    assert packed == ref_packed and stride == ref_stride
    if not packed:
        assert len(piece) == HEADER_BYTES
        return
    assert native.colpack_decode(piece, L, n) == recs.tobytes()
    assert native.colpack_decode(piece, L, n, "scalar") == recs.tobytes()


def test_device_pack2_many_tiles_and_blocks(require_gpu, native):
    """128 * 1024 + 77 rows in 78-row buffers: the pack kernel's tile loop and the statistics kernel's
    row loop both wrap, 128-row tiles begin on rows that restart nothing, and the largest key
    difference sits in the last rows only."""
    rng = np.random.RandomState(3)
    n = 128 * 1024 + 77
    recs = np.empty((n, 104), np.uint8)
    recs[:] = rng.randint(100, 104, size=(n, 104))
    steps = rng.randint(0, 1 << 40, size=n, dtype=np.int64).astype(np.uint64)
    steps[-3:] = (np.uint64(1) << np.uint64(51)) - np.uint64(1)  # rows 28..30 of the last buffer: no restart row
    keys = np.cumsum(steps, dtype=np.uint64)
    recs[:, 3:5] = 0
    for b in range(8):
        recs[:, 5 + b] = ((keys >> np.uint64(56 - 8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    raw = recs.tobytes()
    piece, packed, stride = native.gpu_colpack2_encode([raw], 104, 78, 3, 10)[0]
    want = native.colpack2_encode(raw, 104, 78, 3, 10)
    assert packed and piece[12] & 2  # delta
    assert piece[:HEADER_BYTES] == want[:HEADER_BYTES]
    assert piece == want
    # 94 columns of 2 bits; the differences need 51 bits, which only the last rows set
    assert stride == (188 + 51 + 7) // 8
    assert native.colpack_decode(piece, 104, n) == raw
    recs[-3:, 3:13] = recs[-4, 3:13]  # without them: 40 bits
    piece, packed, stride = native.gpu_colpack2_encode([recs.tobytes()], 104, 78, 3, 10)[0]
    assert packed and stride == (188 + 40 + 7) // 8
    assert piece == native.colpack2_encode(recs.tobytes(), 104, 78, 3, 10)
