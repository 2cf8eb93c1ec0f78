"""The opt-in FASTQ checks of ``execute_demultiplexing(..., _check=True)``: the rule bits and the messages every file
pipeline raises with (core._demux, nativeio.demux_native, deviceio.demux_device, deviceio.demux_device_dealt).
include/biodemux_hip.h has the contract (bdx_fq_check_device, bdx_fq_check_pair_device); the rules themselves are
evaluated by csrc/bdx_fastq.hip, by csrc/bdx_io.cpp and, written out in Python, by core._demux."""
from __future__ import annotations

from .hipabi import BdxError

HEADER, PLUS, LENGTH = 1, 2, 4
ALL_RULES = HEADER | PLUS | LENGTH


def read_name(header: bytes) -> bytes:
    """The name of a header line: its bytes after the first one up to the first ' ' or '\\t' (or the line's end), with one
    trailing "/1" or "/2" dropped."""
    token = header[1:]
    for k, b in enumerate(token):
        if b in (0x20, 0x09):
            token = token[:k]
            break
    return token[:-2] if token[-2:] in (b"/1", b"/2") else token


def reason(broken: int, seq_len: int, qual_len: int) -> str:
    """the first broken rule in bit order, in words"""
    if broken & HEADER:
        return "the header line does not begin with '@'"
    if broken & PLUS:
        return "the third line does not begin with '+'"
    return f"sequence and quality differ in length ({seq_len} against {qual_len})"


def record_error(path: str, record, byte: int, broken: int, seq_len: int, qual_len: int) -> BdxError:
    """``record``: the 1-based record number in the file, or None where the pipeline knows the byte offset alone"""
    where = f"record {record} (at byte {byte} of the text)" if record is not None else f"the record at byte {byte} of the text"
    return BdxError(f"{path}: {where}: {reason(broken, seq_len, qual_len)}")


def pair_error(path1: str, path2: str, record: int, header1: bytes, header2: bytes) -> BdxError:
    return BdxError(f"{path1} and {path2}: record {record}: the read names differ "
                    f"({read_name(header1)!r} against {read_name(header2)!r})")


def count_error(path1: str, path2: str, common: int, first_goes_on: bool) -> BdxError:
    """the two files of a pair hold different numbers of records: ``common`` in both, then one of them goes on"""
    longer, shorter = (path1, path2) if first_goes_on else (path2, path1)
    return BdxError(f"{path1} and {path2}: {longer} goes on from record {common + 1}, {shorter} ends after {common} records")
