"""Device zstd decode (csrc/gpu/zstd.hip, one wave per frame) on the hand-built frames of tests/zstd_cases.py and
the libzstd-written vectors of tests/zstd_vectors.py, which libzstd has judged (tests/test_zstd_cases_cpu.py), and
on what the in-tree encoder writes. The binding puts 256 guard bytes of 0xA5 behind every output and fails on a
changed one, so every call here is also a bounds check; the invalid frames return from their launch with a status
word and a reason, as the corrupt-stream tests of the inflate kernel do. XXH64 (csrc/gpu/xxh64.hip) is held against
the pure-Python one.
"""
import zlib

import pytest

from tests import zstd_cases as zc
from tests.test_zstd_codec import all_valid, encoder_inputs

pytestmark = pytest.mark.gpu

INVALID = zc.INVALID + zc.STRICTER
# what the device decode leaves to the host: a partition of more than one frame
SEVERAL = ("skip-before", "skip-between", "skip-after", "two-frames")


@pytest.fixture(scope="module")
def valid(native):
    cases = [c for c in all_valid() if c[0] not in SEVERAL]
    cases += [("enc_" + name, native.zstd_compress(raw), raw) for name, raw in encoder_inputs().items()]
    if len(cases) % native.gpu_zstd_geometry()["waves_per_block"] == 0:
        cases.append(("one-more", zc.frame([zc.raw_block(b"one more", True)]), b"one more"))
    assert len(cases) >= 65  # several workgroups, the last partly filled
    assert max(len(c[2]) for c in cases) <= 300_000
    return cases


def test_zstd_geometry(native):
    g = native.gpu_zstd_geometry()
    assert g["waves_per_block"] == 4 and g["lds_per_wave"] <= 16384
    assert g["literal_scratch"] == 128 * 1024


def test_valid_frames_in_one_launch(require_gpu, native, valid):
    outs, consumed, with_sum, _, launches = native.gpu_zstd_streams([c[1] for c in valid], [len(c[2]) for c in valid])
    for (name, stream, want), out, used in zip(valid, outs, consumed):
        assert out == want, name
        assert used == len(stream), name
    assert with_sum == sum(1 for c in valid if c[1][4] & 4) and with_sum >= 8 and launches == 1


def test_no_checksum_kernel_without_a_checksum_flag(require_gpu, native, valid):
    plain = [c for c in valid if not c[1][4] & 4][:9]
    outs, consumed, with_sum, _, launches = native.gpu_zstd_streams([c[1] for c in plain], [len(c[2]) for c in plain])
    assert outs == [c[2] for c in plain] and with_sum == 0 and launches == 0


def test_valid_frames_one_launch_each(require_gpu, native, valid):
    for name, stream, want in valid:
        outs, consumed, _, _, _ = native.gpu_zstd_streams([stream], [len(want)])
        assert outs == [want] and consumed == [len(stream)], name


def test_valid_frames_with_four_trailing_bytes(require_gpu, native, valid):
    """An IFile checksum behind the frame is not the frame's: consumed = len - 4."""
    streams = [c[1] + zlib.crc32(c[1]).to_bytes(4, "big") for c in valid]
    outs, consumed, _, _, _ = native.gpu_zstd_streams(streams, [len(c[2]) for c in valid])
    for (name, stream, want), out, used in zip(valid, outs, consumed):
        assert out == want and used == len(stream), name


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_frame_raises(require_gpu, native, name):
    """One launch per case; it returns with the frame's status set (every check is a bounds test ahead of the
    access), and the guards behind the output are untouched."""
    stream, cap = {c[0]: (c[1], c[2]) for c in INVALID}[name]
    with pytest.raises(Exception, match="corrupt|truncated|checksum|dictionary"):
        native.gpu_zstd_streams([stream], [cap])


def test_dictionary_is_refused_by_name(require_gpu, native):
    stream = {c[0]: c[1] for c in INVALID}["dictionary-id"]
    with pytest.raises(Exception, match="needs a dictionary"):
        native.gpu_zstd_streams([stream], [100])


def test_invalid_frame_beside_valid_ones(require_gpu, native, valid):
    """A refused frame in a workgroup does not disturb its neighbours' outputs: the error names it."""
    bad = {c[0]: c[1] for c in INVALID}["offset-before-start"]
    streams = [valid[0][1], bad, valid[1][1], valid[2][1], valid[3][1]]
    raws = [len(valid[0][2]), 4096, len(valid[1][2]), len(valid[2][2]), len(valid[3][2])]
    with pytest.raises(Exception, match="map output #1"):
        native.gpu_zstd_streams(streams, raws)


@pytest.mark.parametrize("delta", [-1, 1])
def test_raw_len_off_by_one_raises(require_gpu, native, valid, delta):
    """A raw length one too small (the output would pass it: nothing is written there, the guards say) and one too
    large both raise."""
    picked = [c for c in valid if c[0] in ("offset1-long", "match-ends-output", "raw-131072", "rle-1", "literals-1025",
                                          "words-l3-sum-fcs", "enc_wordcount", "lit-rle-4096")]
    assert len(picked) == 8
    for name, stream, want in picked:
        with pytest.raises(Exception, match="corrupt|decodes to"):
            native.gpu_zstd_streams([stream], [len(want) + delta])


@pytest.mark.parametrize("name", SEVERAL)
def test_more_than_one_frame_is_left_to_the_host(require_gpu, native, name):
    stream, raw = {c[0]: (c[1], c[2]) for c in zc.VALID}[name]
    what = "corrupt zstd frame.*wrong magic" if name == "skip-before" else "holds more than one frame"
    with pytest.raises(Exception, match=what):
        native.gpu_zstd_streams([stream], [len(raw)])


def test_xxh64_against_python(require_gpu, native):
    data = bytes((i * 131 + (i >> 7)) & 0xFF for i in range(5000))
    buffers = [data[:n] for n in (0, 1, 31, 32, 33, 63, 64, 65, 3000, 4999)] + [data[7:7 + 2048], b"\xff" * 96]
    assert native.gpu_xxh64(buffers) == [zc.xxh64(b) for b in buffers]
    assert len(buffers) < 16  # one workgroup's worth and fewer: the last lanes have no range
    many = [data[k:k + 40 + k] for k in range(37)]  # three workgroups, the last partly filled
    assert native.gpu_xxh64(many) == [zc.xxh64(b) for b in many]
