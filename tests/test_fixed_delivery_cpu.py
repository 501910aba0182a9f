"""Host side of the FIXED10 delivery (csrc/gpu/fixed_delivery.{h,cc}): one landed D2H piece, packed
(colpack version 2) or as records, becomes the buffers the sink gets. Every case is compared with plain
slicing of the records into buf_bytes chunks plus the EOF rule: the marker rides in the task's last
buffer when it fits kv_buf and follows in a 2-byte buffer of its own when it does not. A packed piece
whose header fails a check raises and delivers nothing; with an empty sink the piece is checked and its
buffers counted, nothing else. Also the stand-alone selftest under ASan + UBSan."""
import os
import shutil
import struct
import subprocess

import pytest

from tests.colpack_cases import terasort_records

L = 104
EOF = b"\xff\xff"
HEADER_BYTES = 640


def expected(raw: bytes, buf_bytes: int, kv_buf: int, last: bool):
    out = [raw[o:o + buf_bytes] for o in range(0, len(raw), buf_bytes)]
    if last:
        if out and len(out[-1]) + 2 <= kv_buf:
            out[-1] += EOF
        else:
            out.append(EOF)
    return out


def packed_piece(native, raw: bytes, buf_records: int) -> bytes:
    piece = native.colpack2_encode(raw, L, buf_records, 3, 10)
    assert len(piece) > HEADER_BYTES  # generator values 'A'..'Z': packed, not raw
    return piece


RECS = terasort_records(400, seed=7)


def _raw(n: int) -> bytes:
    return RECS[:n].tobytes()


# (records, buf_records, kv_buf, last)
SHAPES = {
    "312_records_buf_78": (312, 78, 8192, False),
    "one_record": (1, 78, 8192, False),
    "short_last_buffer": (300, 78, 8192, False),
    "last_eof_fits": (300, 78, 8192, True),
    "last_full_buffer_eof_fits_kv": (312, 78, 8192, True),  # 78 * 104 + 2 <= 8192
    "last_exactly_full_eof_separate": (312, 78, 78 * L, True),  # kv_buf a multiple of 104: no room
    "last_one_record": (1, 78, 8192, True),
    "buffer_of_one_record": (5, 1, L, True),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_packed_piece_delivers_the_sliced_records(native, name):
    n, buf_records, kv_buf, last = SHAPES[name]
    raw = _raw(n)
    piece = packed_piece(native, raw, buf_records)
    got = native.fixed_delivery_piece(piece, len(raw), buf_records * L, kv_buf, True, last)
    assert got == expected(raw, buf_records * L, kv_buf, last)
    if name == "last_exactly_full_eof_separate":
        assert got[-1] == EOF and len(got) == 5
    if name == "last_eof_fits":
        assert got[-1].endswith(EOF) and len(got) == 4


@pytest.mark.parametrize("name", list(SHAPES))
def test_unpacked_piece_delivers_the_same_buffers(native, name):
    n, buf_records, kv_buf, last = SHAPES[name]
    raw = _raw(n)
    got = native.fixed_delivery_piece(raw, len(raw), buf_records * L, kv_buf, False, last)
    assert got == expected(raw, buf_records * L, kv_buf, last)


def test_raw_records_travel_unpacked(native):
    """Value bytes 0..255: colpack2_encode gives a header-only (raw) piece, the sender ships the records."""
    import numpy as np
    recs = RECS[:200].copy()
    recs[:, 14:] = np.random.RandomState(3).randint(0, 256, size=(200, 90))
    raw = recs.tobytes()
    assert len(native.colpack2_encode(raw, L, 78, 3, 10)) == HEADER_BYTES
    got = native.fixed_delivery_piece(raw, len(raw), 78 * L, 8192, False, True)
    assert got == expected(raw, 78 * L, 8192, True)


def test_eof_alone(native):
    assert native.fixed_delivery_piece(b"", 0, 78 * L, 8192, False, True) == [EOF]
    assert native.fixed_delivery_piece(b"", 0, 78 * L, 8192, False, False) == []


def _patched(piece: bytes, off: int, fmt: str, value) -> bytes:
    b = bytearray(piece)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def test_rejected_pieces_raise_and_deliver_nothing(native):
    raw = _raw(312)
    piece = packed_piece(native, raw, 78)
    args = (len(raw), 78 * L, 8192, True, True)
    assert native.fixed_delivery_piece(piece, *args) == expected(raw, 78 * L, 8192, True)
    magic = struct.unpack_from("<I", piece, 0)[0]
    with pytest.raises(RuntimeError, match="bad magic"):
        native.fixed_delivery_piece(_patched(piece, 0, "<I", magic ^ 0x100), *args)
    with pytest.raises(RuntimeError, match="record count"):  # the receiver expects 311 records
        native.fixed_delivery_piece(piece, 311 * L, 78 * L, 8192, True, True)
    with pytest.raises(RuntimeError, match="record count"):  # the header claims 313
        native.fixed_delivery_piece(_patched(piece, 16, "<Q", 313), *args)
    with pytest.raises(RuntimeError, match="exceed the piece's length"):
        native.fixed_delivery_piece(piece[:len(piece) - 64], *args)
    with pytest.raises(RuntimeError, match="shorter than its header"):
        native.fixed_delivery_piece(piece[:HEADER_BYTES - 1], *args)
    import numpy as np
    noise = np.random.RandomState(4).randint(0, 256, size=(312, L)).astype(np.uint8).tobytes()
    header_only = native.colpack2_encode(noise, L, 78, 3, 10)
    assert len(header_only) == HEADER_BYTES
    with pytest.raises(RuntimeError, match="not marked packed"):
        native.fixed_delivery_piece(header_only, *args)
    with pytest.raises(RuntimeError, match="another length"):  # an unpacked piece must be its records
        native.fixed_delivery_piece(raw[:-L], len(raw), 78 * L, 8192, False, True)


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_empty_sink_counts_the_same_buffers(native, name, packed):
    """No sink (the flagship's --sink none): the piece is checked and counted, nothing is unpacked."""
    n, buf_records, kv_buf, last = SHAPES[name]
    raw = _raw(n)
    piece = packed_piece(native, raw, buf_records) if packed else raw
    args = (piece, len(raw), buf_records * L, kv_buf, packed, last)
    with_sink = native.fixed_delivery_piece(*args)
    c = native.fixed_delivery_piece(*args, deliver=False)
    assert c["buffers"] == len(with_sink) == len(expected(raw, buf_records * L, kv_buf, last))
    assert c["eof_sent"] == last == (bool(with_sink) and with_sink[-1].endswith(EOF))
    assert c["unpack_ms"] == 0


def test_empty_sink_still_rejects_a_bad_header(native):
    raw = _raw(312)
    piece = packed_piece(native, raw, 78)
    args = (len(raw), 78 * L, 8192, True, True)
    assert native.fixed_delivery_piece(piece, *args, deliver=False)["buffers"] == 4
    magic = struct.unpack_from("<I", piece, 0)[0]
    with pytest.raises(RuntimeError, match="bad magic"):
        native.fixed_delivery_piece(_patched(piece, 0, "<I", magic ^ 0x100), *args, deliver=False)
    with pytest.raises(RuntimeError, match="record count"):
        native.fixed_delivery_piece(piece, 311 * L, 78 * L, 8192, True, True, deliver=False)
    with pytest.raises(RuntimeError, match="another length"):
        native.fixed_delivery_piece(raw[:-L], len(raw), 78 * L, 8192, False, True, deliver=False)


def test_packed_copy_len_accepts_header_to_bound(native):
    """The one check of a packed length the device reported, before it becomes a copy length: at least
    a header, at most the piece's bound, at most a ring slot."""
    lay = (8192, 32 << 10, 4, 2)
    bound = native.fixed_delivery_layout(*lay)["bound_full"]  # a piece of 312 records
    assert bound > HEADER_BYTES
    for ok in (HEADER_BYTES, bound):
        assert native.fixed_delivery_packed_copy_len(*lay, ok, 312) == ok
    for bad in (HEADER_BYTES - 1, bound + 1):
        with pytest.raises(RuntimeError, match="packed length"):
            native.fixed_delivery_packed_copy_len(*lay, bad, 312)
    tiny = (104, 104, 2, 2)  # bound and slot 832
    assert native.fixed_delivery_packed_copy_len(*tiny, 832, 1) == 832
    with pytest.raises(RuntimeError, match="packed length"):
        native.fixed_delivery_packed_copy_len(*tiny, 833, 1)


def test_pack_key_values(native, monkeypatch):
    monkeypatch.delenv("UDA_DELIVERY_PACK", raising=False)
    assert [native.delivery_pack_version(v) for v in ("auto", "v1", "off", "on", "")] == [2, 1, 0, -1, -1]
    monkeypatch.setenv("UDA_DELIVERY_PACK", "0")
    assert [native.delivery_pack_version(v) for v in ("auto", "v1", "off", "bogus")] == [0, 0, 0, -1]


@pytest.mark.parametrize("key,value", [("mapred.uda.gpu.delivery.pack", "v3"), ("mapred.uda.gpu.delivery.piece.bytes", "-1")])
def test_bad_key_value_fails_init(key, value):
    """A GPU-backend reduce task reads both keys at INIT (no device is touched before that fails)."""
    from uda_amd.bridge import UdaConsumer
    from uda_amd.utils import datagen
    with pytest.raises(Exception, match=key.replace(".", r"\.")):
        UdaConsumer(1, "job_1_0701", "attempt_job_1_0701_r_000000_0", datagen.TEXT,
                    conf={"mapred.uda.merge.backend": "gpu", key: value})


def test_layout_sizes_slots_from_the_bound(native, monkeypatch):
    """A ring slot holds the piece or its packed bound, whichever is larger; with pack off the ring is
    slots * piece, as before; prewarm and task share this one function."""
    off = native.fixed_delivery_layout(8192, 32 << 10, 4, 0)
    assert off["piece"] == 312 * L and off["slot_bytes"] == off["piece"] and off["ring_bytes"] == 4 * 312 * L
    v2 = native.fixed_delivery_layout(8192, 32 << 10, 4, 2)
    assert v2["slot_bytes"] >= max(v2["piece"], v2["bound_full"]) and v2["slot_bytes"] % 64 == 0
    assert v2["ring_bytes"] == 4 * v2["slot_bytes"] + 2 * v2["staging_bytes"] and v2["staging_bytes"] >= 8192 + 16
    # a one-record piece is longer packed (768 bytes) than plain (104): the slot follows the bound
    tiny = native.fixed_delivery_layout(104, 104, 2, 2)
    assert tiny["piece"] == 104 and tiny["bound_full"] == 832 and tiny["slot_bytes"] == 832
    assert native.fixed_delivery_layout(104, 104, 2, 1)["bound_full"] == 768


def test_fixed_delivery_native_selftest_under_sanitizers(tmp_path):
    """tests/native/fixed_delivery_selftest.cc, a program of its own, built with csrc/gpu/fixed_delivery.cc
    and csrc/codec/colpack.cc under ASan + UBSan: the cases above on exact-size heap buffers plus pieces
    of 1..400 records against buf_records 1, 13 and 78."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fixed_delivery_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc"), "-I" + os.path.join(root, "csrc", "gpu"),
                    os.path.join(root, "tests", "native", "fixed_delivery_selftest.cc"),
                    os.path.join(root, "csrc", "gpu", "fixed_delivery.cc"),
                    os.path.join(root, "csrc", "codec", "colpack.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
