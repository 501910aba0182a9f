"""colpack device kernels (csrc/gpu/colpack.hip: stats, plan, pack) on small device arrays: the bytes
they write, header and padding included, equal the host reference encoder's byte for byte, and
host-decoding them gives back the input. Same cases as tests/test_colpack_cpu.py."""
import numpy as np
import pytest

from tests.colpack_cases import BUF_RECORDS, HEADER_BYTES, cases, np_encode

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def device_pieces(require_gpu, native):
    """name -> (piece bytes, packed, stride) from one launch of the three kernels per record length:
    the pieces of a launch differ in size, as a round's D2H pieces do."""
    by_len = {}
    for name, (recs, _) in CASES.items():
        by_len.setdefault(recs.shape[1], []).append(name)
    out = {}
    for L, names in by_len.items():
        res = native.gpu_colpack_encode([CASES[n][0].tobytes() for n in names], L, BUF_RECORDS)
        out.update(zip(names, res))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_device_pack_equals_host_encoder(native, device_pieces, name):
    recs, expect = CASES[name]
    n, L = recs.shape
    piece, packed, stride = device_pieces[name]
    want = native.colpack_encode(recs.tobytes(), L, BUF_RECORDS)
    assert want == np_encode(recs, BUF_RECORDS)[0]
    assert piece[:HEADER_BYTES] == want[:HEADER_BYTES]
    assert piece == want
    if expect == "raw":
        assert not packed and len(piece) == HEADER_BYTES
        return
    assert packed and (expect is None or stride <= expect)
    assert native.colpack_decode(piece, L, n) == recs.tobytes()
    assert native.colpack_decode(piece, L, n, "scalar") == recs.tobytes()


def test_device_pack_many_tiles_and_blocks(require_gpu, native):
    """More rows than one launch's grid covers in one stride, so the pack kernel's tile loop and the
    statistics kernel's row loop both wrap; the extremes sit in the last rows only."""
    rng = np.random.RandomState(3)
    n = 128 * 1024 + 77  # pack grid: 1024 workgroups of 128-row tiles
    recs = np.empty((n, 104), np.uint8)
    recs[:] = rng.randint(100, 104, size=(n, 104))
    recs[-1, :] = 0
    recs[-2, :] = 255
    piece, packed, stride = native.gpu_colpack_encode([recs.tobytes()], 104, BUF_RECORDS)[0]
    assert not packed and stride == 104  # 8 bits everywhere: raw
    recs[-1, :] = 100
    recs[-2, :] = 107
    raw = recs.tobytes()
    piece, packed, stride = native.gpu_colpack_encode([raw], 104, BUF_RECORDS)[0]
    assert packed and stride == 39  # 3 bits per column: 13 groups of 3 bytes
    assert piece == native.colpack_encode(raw, 104, BUF_RECORDS)
    assert native.colpack_decode(piece, 104, n) == raw
