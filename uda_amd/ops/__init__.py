"""Python views of the native data-path operations.

merge_runs(runs, key_class, device="gpu"|"cpu") merges sorted IFile runs (byte strings, each the
raw partition stream of one map output) and returns (merged record bytes, buffer cut offsets).
The GPU path runs the HIP kernels F1 (record index), F2 (key normalize), F3 (merge-path merge
tree) and F4 (scan + gather) of csrc/gpu; the CPU path is the reference heap merge. There is no
silent fallback: device="gpu" raises when no HIP device or extension is available.
"""
from __future__ import annotations

from .._native import native

EOF_MARKER = b"\xff\xff"
last_stats: dict = {}  # timing of the most recent merge_runs call (device merge excludes H2D/D2H)


def merge_runs(runs: list[bytes], key_class: str, device: str = "gpu", kv_buf: int = 1 << 20,
               gpu_index: int = 0, combine: str = "none", key_order: str = "reference"):
    """key_order: a value of mapred.uda.key.order. "reference": the reference's three comparators (numeric
    keys by memcmp). "hadoop": Byte/Short/Int/Long/VInt/VLong/Float/DoubleWritable keys in the order of their
    Hadoop comparators (uda/compare.h: key_sortable); a key of the wrong length raises.
    combine: "none" or an op of mapred.uda.merge.combine: equal keys are folded into the first record of
    their group, on the device (csrc/gpu/combine.hip) or by the host reference.
      sum.int, sum.long                      4 / 8-byte big-endian values, wrapping sum
      min.int, max.int, min.long, max.long   the same values, signed minimum / maximum
      sum.vint, sum.vlong                    one Hadoop VInt / VLong per value; the sum is re-encoded
                                             canonically, so a delivered record can change length"""
    n = native()
    if device == "gpu":
        if n.device_count() <= 0:
            raise RuntimeError("merge_runs(device='gpu'): no HIP device visible")
        merged, cuts, _records, _passes, merge_ms, serial, records_in = n.gpu_merge_runs(
            list(runs), key_class, kv_buf - 2, gpu_index, combine, key_order)
        last_stats.update(device="gpu", records=_records, passes=_passes, merge_ms=merge_ms, f1_serial_runs=serial,
                          records_in=records_in)
        return merged, cuts
    if device == "cpu":
        out, lens = n.cpu_merge(list(runs), key_class, kv_buf, combine, key_order)
        # cpu_merge already appended the EOF marker and packed greedily
        body = out[:-2]
        cuts, pos = [0], 0
        for ln in lens:
            pos = min(pos + ln, len(body))
            if pos != cuts[-1]:
                cuts.append(pos)
        return body, cuts
    raise ValueError(f"unknown device {device!r}")


def merge_runs_streamed(runs: list[bytes], key_class: str, kv_buf: int = 1 << 20, round_bytes: int = 256 << 20,
                        gpu_index: int = 0, combine: str = "none", key_order: str = "reference"):
    """The device merge handed over in key-range rounds of about round_bytes of input, as a reduce task
    receives it. Returns (merged record bytes, cuts, stats): stats has records, records_in, held_records and
    rounds, a list of (records, cuts of that round) per hand-over. Under combine a round ends on a group
    boundary: an open last group is carried into the next round (held_records counts those elements)."""
    n = native()
    if n.device_count() <= 0:
        raise RuntimeError("merge_runs_streamed: no HIP device visible")
    merged, cuts, records, records_in, rounds, held = n.gpu_merge_runs_streamed(
        list(runs), key_class, kv_buf - 2, round_bytes, gpu_index, combine, key_order)
    return merged, cuts, dict(records=records, records_in=records_in, rounds=rounds, held_records=held)


def _key_kind(n, key_class: str, key_order: str) -> int:
    kind = n.key_kind_ordered(key_class, key_order)
    if kind < 0:
        raise ValueError(f"unsupported key class {key_class!r} under key_order={key_order!r}")
    return kind


def plan_generic_rounds(runs: list[bytes], key_class: str, round_bytes: int, key_order: str = "reference",
                        misalign: int = 0, gpu_index: int = 0) -> dict:
    """The key-range round plan of the device-generic merge (csrc/gpu/generic_rounds.h) for whole runs:
    rounds, pos[run][0..rounds] (byte offsets), bounds (the rounds - 1 strings the runs were split by) and
    max_round_bytes. Every run starts `misalign` bytes past a 256-byte-aligned device address."""
    n = native()
    if n.device_count() <= 0:
        raise RuntimeError("plan_generic_rounds: no HIP device visible")
    return n.gpu_plan_generic_rounds(list(runs), _key_kind(n, key_class, key_order), round_bytes, misalign, gpu_index)


def plan_progressive_split(windows: list[bytes], avail: list[int], final: list[bool], key_class: str,
                           key_order: str = "reference", misalign: int = 0, gpu_index: int = 0) -> dict:
    """The split of a progressive merge phase: windows[k] are the bytes of run k not merged yet, the first
    avail[k] of them landed; final[k]: the window reaches the run's end. Returns complete (end of the last
    whole landed record), split (the bytes of each window safe to merge now), bounded and bound."""
    n = native()
    if n.device_count() <= 0:
        raise RuntimeError("plan_progressive_split: no HIP device visible")
    return n.gpu_plan_progressive_split(list(windows), list(avail), [bool(f) for f in final],
                                        _key_kind(n, key_class, key_order), misalign, gpu_index)


def buffers(merged: bytes, cuts: list[int]) -> list[bytes]:
    """Split a merged stream at the cut offsets into delivery buffers, EOF in the last one."""
    out = [merged[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    if out:
        out[-1] += EOF_MARKER
    else:
        out = [EOF_MARKER]
    return out
