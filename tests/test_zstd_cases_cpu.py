"""tests/zstd_cases.py and tests/zstd_vectors.py held against libzstd itself (the system library through ctypes,
where it loads: the live assertions skip where it does not), and the coverage the vectors must bring, measured
with native.zstd_decoder_stats: the in-tree encoder writes Raw literals and Predefined-mode sequences only, so
every other path of the decoders is reached through the vectors."""
import ctypes

import pytest

from tests import zstd_cases as zc
from tests.zstd_vectors import VECTORS, raw_of


def load_libzstd():
    for name in ("libzstd.so.1", "libzstd.so"):
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        for f in ("ZSTD_decompress", "ZSTD_compressBound", "ZSTD_compress"):
            getattr(lib, f).restype = ctypes.c_size_t
        lib.ZSTD_isError.restype = ctypes.c_uint
        return lib
    return None


LIB = load_libzstd()
live = pytest.mark.skipif(LIB is None, reason="no libzstd on this machine")


def lib_decompress(stream, cap):
    """The decoded bytes, or None where libzstd refuses the stream."""
    out = ctypes.create_string_buffer(max(cap, 1))
    r = LIB.ZSTD_decompress(out, ctypes.c_size_t(cap), stream, ctypes.c_size_t(len(stream)))
    return None if LIB.ZSTD_isError(ctypes.c_size_t(r)) else out.raw[:r]


def lib_compress(raw, level=3):
    cap = LIB.ZSTD_compressBound(ctypes.c_size_t(len(raw)))
    out = ctypes.create_string_buffer(cap)
    r = LIB.ZSTD_compress(out, ctypes.c_size_t(cap), raw, ctypes.c_size_t(len(raw)), level)
    assert not LIB.ZSTD_isError(ctypes.c_size_t(r))
    return out.raw[:r]


@pytest.fixture(scope="module")
def vector_raws():
    return {v[0]: raw_of(v[1]) for v in VECTORS}


@live
@pytest.mark.parametrize("case", zc.VALID + zc.SHAPES + zc.BEYOND_WINDOW, ids=lambda c: c[0])
def test_libzstd_decodes_the_valid_cases(case):
    name, stream, raw = case
    assert lib_decompress(stream, len(raw)) == raw


@live
@pytest.mark.parametrize("case", zc.INVALID, ids=lambda c: c[0])
def test_libzstd_refuses_the_invalid_cases(case):
    name, stream, cap = case
    assert lib_decompress(stream, cap) is None


@live
def test_libzstd_takes_what_the_format_forbids_and_we_do_not(native):
    """The known places where the decoders here are stricter than libzstd 1.4.8's one-shot call: each is outside
    the format, so no valid frame is affected (docs/ARCHITECTURE.md lists them)."""
    whys = set()
    for name, stream, cap in zc.STRICTER:
        assert lib_decompress(stream, cap) is not None, name
        with pytest.raises(ValueError, match="corrupt zstd frame") as e:
            native.zstd_decompress(stream, cap)
        whys.add(str(e.value).split(": ", 1)[1])
    assert whys == {"block larger than min(window, 128 KiB)", "block regenerates more than its limit",
                    "sequence bitstream not used up", "sequence bitstream ends early"}


@live
def test_libzstd_decodes_the_vectors(vector_raws):
    for name, spec, level, checksum, content_size, frame in VECTORS:
        assert lib_decompress(frame, len(vector_raws[name])) == vector_raws[name], name


@live
def test_python_xxh64_against_checksums_libzstd_wrote(vector_raws):
    seen = 0
    for name, spec, level, checksum, content_size, frame in VECTORS:
        if checksum:
            assert int.from_bytes(frame[-4:], "little") == zc.xxh64(vector_raws[name]) & 0xFFFFFFFF, name
            seen += 1
    assert seen >= 8


def test_python_xxh64_known_values():
    assert zc.xxh64(b"") == 0xEF46DB3751D8E999
    assert zc.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert zc.xxh64(b"abc") == 0x44BC2CF5AD770999


def test_vector_flags_are_in_the_frames():
    for name, spec, level, checksum, content_size, frame in VECTORS:
        d = frame[4]
        assert bool(d & 4) == checksum, name
        assert (bool(d >> 6) or bool(d & 0x20)) == content_size, name
    assert {v[2] for v in VECTORS} >= {1, 3, 9, 19}


def test_vectors_cover_the_format(native, vector_raws):
    blocks, literals, weights = {}, {}, {}
    modes = {t: {} for t in ("ll", "of", "ml")}
    most_blocks = far = 0
    for name, spec, level, checksum, content_size, frame in VECTORS:
        st = native.zstd_decoder_stats(frame, len(vector_raws[name]))
        for total, part in ((blocks, st["blocks"]), (literals, st["literals"]), (weights, st["weights"])):
            for k, v in part.items():
                total[k] = total.get(k, 0) + v
        for t in modes:
            for k, v in st["modes"][t].items():
                modes[t][k] = modes[t].get(k, 0) + v
        most_blocks = max(most_blocks, st["max_frame_blocks"])
        far = max(far, st["max_offset"])
    assert all(blocks[k] > 0 for k in ("raw", "rle", "compressed")), blocks
    assert all(literals[k] > 0 for k in ("raw", "rle", "compressed", "treeless", "streams1", "streams4")), literals
    assert weights["direct"] > 0 and weights["fse"] > 0, weights
    for t in modes:
        assert all(modes[t][k] > 0 for k in ("predefined", "rle", "fse", "repeat")), (t, modes[t])
    assert most_blocks >= 3
    assert far > 128 * 1024


def test_vector_module_is_small():
    import os
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "zstd_vectors.py")) < 200 * 1024


def test_literal_section_vectors_have_the_sizes_their_names_say(native, vector_raws):
    """All literals and no sequence: the section's regenerated size is the frame's, on both sides of the 1-stream /
    4-stream and size-format boundaries and with uneven fourth streams."""
    sizes = set()
    for name, spec, level, checksum, content_size, frame in VECTORS:
        if name.startswith("literals-"):
            st = native.zstd_decoder_stats(frame, len(vector_raws[name]))
            assert st["sequences"] == 0 and st["literals"]["compressed"] == 1 and st["blocks"] == {"raw": 0, "rle": 0, "compressed": 1}
            assert len(vector_raws[name]) == int(name.split("-")[1])
            sizes.add(len(vector_raws[name]))
    assert sizes == {255, 256, 1023, 1024, 1025, 1026}
