"""execute_demultiplexing — the drop-in API surface (BioDemuX.jl src/core.jl:360, :500).

Same positional arguments, keyword names, defaults and file contract as the reference; the
per-read classification (worker_task's loop, core.jl:243-267) is ONE C-ABI call per batch on
the MI355X instead of nthreads() Julia workers.  Reader and writer here are plain host code
that keeps the reference's observable behaviour (record framing, naming, ordering, append
mode, trimming of R1 only); they are the "next" rows of SURVEY §8(f), not the hot path.
"""
from __future__ import annotations

import datetime as _dt
import gzip
import operator
import os
import re
import sys
from typing import Callable, Dict, List, Optional

import numpy as np

from .classification import DemuxStats, filename_for, merge_stats_tables
from .config import DemuxConfig, build_config
from .fileio import read_fastq
from . import checks, deviceio, nativeio
from .hipabi import HipClassifier, load_library
from .outputs import OutputLayout
from .reporting import canonical_duration, generate_summary_report

_PREFIX_RE = re.compile(r"\.fastq(\.gz)?$")

# Reads handed to the device per C-ABI call.  The reference hands 4000-read chunks to each
# worker (chunk_size); a GPU wants >= 10^5 reads per launch (256 CUs x 8 waves x 64 lanes).
DEFAULT_BATCH_READS = 1 << 19  # reads per C-ABI call of the file pipeline (the kernels are at full speed from ~10^5 reads on; smaller batches fill the pipeline sooner)


def _records(io, offsets: Optional[list] = None):
    """FASTQ framing of reader_task (core.jl:96-101): while !eof, four readline() calls; a
    truncated last record is padded with empty lines exactly as readline at EOF returns "".
    ``offsets`` (a list, for ``_check``) receives the byte offset of every record's first line in the text."""
    data = io.read()
    if not data:
        return
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # data ended with '\n': no further line exists
    if offsets is not None:
        at = 0
        for i, ln in enumerate(lines):
            if i % 4 == 0:
                offsets.append(at)
            at += len(ln) + 1
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]  # readline strips "\r\n"
    n = len(lines)
    for i in range(0, n, 4):
        rec = lines[i:i + 4]
        while len(rec) < 4:
            rec.append(b"")
        yield rec


def _broken_rules(rec) -> int:
    """the record rules of ``_check`` (include/biodemux_hip.h, bdx_fq_check_device) on one framed record"""
    h, s, p, q = rec
    return ((checks.HEADER if h[:1] != b"@" else 0) | (checks.PLUS if p[:1] != b"+" else 0)
            | (checks.LENGTH if len(s) != len(q) else 0))


class _Writer:
    """writer_task (core.jl:118-224): lazily opened per-file handles in append mode, gzip when
    config.gzip_output or the name ends with .gz, records written as h\\ns\\np\\nq\\n."""

    def __init__(self, output_dir: str, config: DemuxConfig):
        self.dir = output_dir
        self.config = config
        self.handles: Dict[str, object] = {}

    def get(self, filename: str):
        h = self.handles.get(filename)
        if h is None:
            path = os.path.join(self.dir, filename)
            should_gzip = self.config.gzip_output or path.lower().endswith(".gz")  # core.jl:127
            h = gzip.open(path, "ab") if should_gzip else open(path, "ab")
            self.handles[filename] = h
        return h

    def write_entry(self, filename: str, h: bytes, s: bytes, p: bytes, q: bytes):
        self.get(filename).write(b"".join((h, b"\n", s, b"\n", p, b"\n", q, b"\n")))  # core.jl:134-136

    def close(self):
        for h in self.handles.values():
            h.close()
        self.handles.clear()


def _log(msg: str):
    print(f"[{_dt.datetime.now().strftime('%H:%M:%S')}] {msg}", file=sys.stderr)


def _demux(fastq1: str, fastq2: Optional[str], config: DemuxConfig, output_directory: str, prefix1: str,
           prefix2: str, classifiers: list, batch_reads: int, on_batch=None,
           batches_per_device: Optional[list] = None, check: bool = False, timings: Optional[dict] = None) -> None:
    """Batch k goes to classifier k % N of the N ``classifiers``, one batch at a time (the plain statement of what
    nativeio's dealer does with threads); ``batches_per_device`` receives the counts.  ``check``: every batch is held to
    the record rules (file 1's records, then file 2's) and a paired one to the pair rule before it is classified, and a
    pair of files with different numbers of records is refused after the last common batch; ``timings`` then receives
    check_s and checked_records."""
    writer = _Writer(output_directory, config)
    streams = OutputLayout(config, output_directory, prefix1, prefix2, fastq2 is not None).streams
    dealt = [0] * len(classifiers)
    at1: Optional[list] = [] if check else None  # byte offsets of the records' first lines
    at2: Optional[list] = [] if check and fastq2 is not None else None
    done = [0, 0.0]  # records flushed so far, seconds in the checks

    def check_batch(r1: List[list], r2: Optional[List[list]]):
        t0 = _dt.datetime.now()
        for path, recs, at in ((fastq1, r1, at1), (fastq2, r2, at2)):
            for i, rec in enumerate(recs or ()):
                broken = _broken_rules(rec)
                if broken:
                    raise checks.record_error(path, done[0] + i + 1, at[done[0] + i], broken, len(rec[1]), len(rec[3]))
        for i, (a, b) in enumerate(zip(r1, r2 or ())):
            if checks.read_name(a[0]) != checks.read_name(b[0]):
                raise checks.pair_error(fastq1, fastq2, done[0] + i + 1, a[0], b[0])
        done[1] += (_dt.datetime.now() - t0).total_seconds()

    def flush(r1: List[list], r2: Optional[List[list]]):
        if not r1:
            return
        if check:
            check_batch(r1, r2)
            done[0] += len(r1)
        seqs = [rec[1] for rec in r1]
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        blob = np.frombuffer(b"".join(seqs), dtype=np.uint8) if off[-1] else np.zeros(0, dtype=np.uint8)
        k = sum(dealt) % len(classifiers)
        out = classifiers[k].classify(blob, off)  # <- the hot path: one C-ABI call per batch
        dealt[k] += 1
        if on_batch is not None:
            on_batch(out)
        bc1, bc2, ks, ke = out["bc1"], out["bc2"], out["keep_start"], out["keep_end"]
        for i, (h1, s1, p1, q1) in enumerate(r1):
            filename = filename_for(config, int(bc1[i]), int(bc2[i]))
            for src, prefix, trim in streams:  # core.jl:175-196
                if src == 1:
                    writer.write_entry(prefix + "." + filename, *r2[i])
                    continue
                if trim and ks[i] != -1:  # core.jl:250-254, :162-173
                    a = max(int(ks[i]), 1)
                    b = min(int(ke[i]), len(s1))
                    if a <= b:
                        s1 = s1[a - 1:b]
                        q1 = q1[a - 1:b]
                    else:
                        s1 = b""
                        q1 = b""
                writer.write_entry(prefix + "." + filename, h1, s1, p1, q1)

    try:
        with read_fastq(fastq1) as io1:
            if fastq2 is not None:
                with read_fastq(fastq2) as io2:  # lock-step pairs, core.jl:48-75
                    b1: List[list] = []
                    b2: List[list] = []
                    it1, it2 = _records(io1, at1), _records(io2, at2)
                    for rec1, rec2 in zip(it1, it2):
                        b1.append(rec1)
                        b2.append(rec2)
                        if len(b1) >= batch_reads:
                            flush(b1, b2)
                            b1, b2 = [], []
                    flush(b1, b2)
                    if check:
                        next(it1, None), next(it2, None)  # (zip never started the second reader of an empty first file)
                    if check and len(at1) != len(at2):  # (without it: the lock-step stop at the shorter file, core.jl:48)
                        raise checks.count_error(fastq1, fastq2, min(len(at1), len(at2)), len(at1) > len(at2))
            else:
                b1 = []
                for rec1 in _records(io1, at1):
                    b1.append(rec1)
                    if len(b1) >= batch_reads:
                        flush(b1, None)
                        b1 = []
                flush(b1, None)
    finally:
        writer.close()
        if batches_per_device is not None:
            batches_per_device[:] = dealt
        if check and timings is not None:
            timings.update(check_s=done[1], checked_records=done[0] * (2 if fastq2 is not None else 1))


def _device_list(device: int, devices, io: str) -> List[int]:
    """The contexts of a run: ``devices`` (several entries may name one GPU), or ``[device]``."""
    if devices is None:
        return [device]
    if isinstance(devices, (str, bytes)):
        raise TypeError("devices must be a sequence of HIP device indices, e.g. [0, 1]")
    devs = [operator.index(d) for d in devices]
    if not devs:
        raise ValueError("devices is empty: name at least one HIP device")
    if any(d < 0 for d in devs):
        raise ValueError(f"device indices are >= 0 (got devices={devs})")
    if device != 0:
        raise ValueError("pass either device= or devices=, not both")
    if len(devs) > 1 and io == "device":
        # the device pipeline finds batch k + 1's first record only after batch k's index ran on the device: dealing
        # batches over contexts needs another design, and falling back to the host pipeline would hide that
        raise ValueError("_io='device' drives one device context: batch boundaries are found on the device, so batches "
                         "cannot be dealt over several devices; use _io='native' (or 'auto') with devices=, or "
                         "_io='device-deal', which deals byte spans of a single-end input over the contexts")
    return devs


def _open_classifiers(config: DemuxConfig, devs: List[int], factory) -> list:
    """One context per entry of ``devs``; if one fails to open, the ones already open are closed first."""
    out = []
    try:
        for d in devs:
            out.append(factory(config) if factory else HipClassifier(config, device=d))
    except BaseException:
        _close_all(out)
        raise
    return out


def _close_all(classifiers) -> None:
    """close() every classifier, also when one of them fails; the first failure is raised afterwards."""
    first = None
    for c in classifiers:
        try:
            c.close()
        except BaseException as e:  # noqa: BLE001
            first = first or e
    if first is not None:
        raise first


def execute_demultiplexing(*args, _classifier_factory: Optional[Callable[[DemuxConfig], object]] = None,
                           _batch_reads: int = DEFAULT_BATCH_READS, _io: str = "auto", device: int = 0,
                           devices=None, _timings: Optional[dict] = None, _gzip: str = "host", _gunzip: str = "host",
                           _gzip_level: int = 1, _gunzip_window: Optional[int] = None, _span_bytes: Optional[int] = None,
                           _check: bool = False, **kw):
    """execute_demultiplexing(FASTQ_file, barcode_file, output_directory; kwargs...)      core.jl:500
    execute_demultiplexing(FASTQ_file1, FASTQ_file2, barcode_file, output_directory; ...)  core.jl:360

    Keyword arguments and defaults are the reference's (core.jl:365-391 / :504-528).
    ``_io`` selects the host-side reader/writer: "native" (csrc/bdx_io.cpp, threads), "python" (the
    plain reference implementation below), "auto" (native when the library was built) or "device" (index, pack,
    split by output file and gather on the GPU, deviceio.py: needs the HIP classifier).
    ``_io="device-deal"`` is the device pipeline dealt over the contexts of ``devices`` by byte spans (deviceio.
    demux_device_dealt): the input is cut into spans of ``_span_bytes`` bytes (an int of at least 16; default
    ``_batch_reads`` x 330 bytes rounded up to 64 KiB, whatever the number of contexts), a record belongs to the span its
    first line starts in, every context takes the next span and runs the whole device pipeline on it, one writer
    appends the blocks in span order.  Same files, counters and reports as ``_io="device"``.  Single-end input only,
    plain or a ``.gz`` inflated by the host (``_gunzip="host"``); ``_gzip="device"`` works at both levels; ``_timings``
    then also holds spans, spans_per_device, span_bytes, devices and phase_wait_s, the busy seconds summed over the contexts.
    (The ValueError for an unknown ``_io`` keeps its earlier wording and does not list "device-deal"; it is a valid value.)
    ``_classifier_factory`` is a test seam: the parity tests on CPU pass the oracle here to
    check this file contract; the product default is the HIP classifier and nothing else.
    ``devices`` (a sequence of HIP device indices, None = ``[device]``): one device context per entry — repeated entries
    put several contexts on one GPU — and the batches are dealt over them (merge_stats over the workers, core.jl:587-599);
    output files, counters and reports are those of one context.  ``_io="device"`` takes a single device.
    ``_timings`` (a dict) receives the busy seconds of the native pipeline's stages (bench.py's end-to-end figure; with
    _io="device": upload_s, device_s, download_s, write_s and batches; with several devices also devices,
    classify_s_per_device and batches_per_device, classify_s being their sum).
    ``_gzip`` selects who compresses gzip output: "host" (zlib on the writer's threads) or "device" (csrc/bdx_deflate.hip:
    the device pipeline deflates each batch's blocks and downloads finished gzip members; needs ``_io="device"``, inert
    when the output is not gzip; _timings then also holds deflate_s, plain_bytes, compressed_bytes and gzip_level).
    ``_gzip_level`` (1 or 2, with ``_gzip="device"`` only) is the device encoder's level: 1 is the fast one, 2 finds
    better matches and writes smaller files (bdx_fq_deflate_level_device).
    ``_gunzip`` selects who inflates a ``.gz`` input: "host" (zlib on host threads, csrc/bdx_io.cpp), "device",
    "device-stream" or "device-window".  "device" is for chains of small tagged members
    (csrc/bdx_inflate.hip: the device pipeline uploads the compressed members and inflates them on the GPU, checking
    every member's CRC-32 and ISIZE there; needs ``_io="device"``; inert for a plain input; a ``.gz`` input must be a
    chain of size-tagged gzip members — BGZF, or what ``_gzip="device"`` writes — of at most 64 KiB each, anything else
    is a ValueError; _timings then also holds inflate_s, compressed_in_bytes and plain_in_bytes, and upload_s covers
    compressed bytes only).  "device-stream" (csrc/bdx_inflate_stream.hip) takes an ORDINARY ``.gz`` input — one gzip
    member or a few, of any size, tagged or not: the whole compressed file is uploaded and inflated on the GPU from
    speculative block starts before the first batch, the text stays resident in device memory (the compressed bytes
    plus three times the plain bytes at the peak; a file that does not fit is a BdxError that says so) and the batches
    are windows into it; needs ``_io="device"``; inert for a plain input; a ``.gz`` input that does not begin with a
    gzip header is a ValueError; _timings then holds inflate_s, compressed_in_bytes, plain_in_bytes and the counters
    stream_members, stream_chunks, stream_confirmed, stream_discarded, stream_no_candidate and stream_longest_segment.
    "device-window" (bdx_fq_inflate_window_*, csrc/bdx_inflate_window_core.h) takes the same ordinary ``.gz`` input
    of ANY size: the compressed file goes through the GPU in windows of ``_gunzip_window`` compressed bytes (an int of
    1024 .. 2^28, rounded up to a multiple of the chunk size; default deviceio.WINDOW_BYTES), each inflated from the
    state the one before ended in while the next one is uploaded, and the text is handed to the batches as it appears:
    device memory follows the window, not the file (deviceio's docstring has the bound).  A member's CRC-32 is known at
    its end only: a refused member raises BdxError naming the file, the member, the compressed offset and the reason
    AFTER the batches of the windows before it were written, as with ``_gunzip="host"`` — not before the first batch,
    as "device-stream" does.  Needs ``_io="device"``; inert for a plain input; a ``.gz`` input that does not begin with
    a gzip header is a ValueError; _timings holds what "device-stream" reports, summed over the windows
    (stream_longest_segment: the maximum), and stream_windows, stream_window_bytes and stream_text_peak_bytes.
    ``_check`` (a bool, default False: the reference checks nothing, and nothing is checked, enqueued or timed without
    it): every batch of every input is held to three record rules after its index and before it is packed and
    classified — line 1 begins with '@', line 3 begins with '+', sequence and quality have the same length — and a
    paired batch to the pair rule: the read names (the header after its first byte up to the first blank, one trailing
    "/1" or "/2" dropped) of record i of both files are equal (include/biodemux_hip.h: bdx_fq_check_device,
    bdx_fq_check_pair_device; csrc/bdx_io.cpp for ``_io="native"``, core._demux for "python").  File 1's records are
    checked first, then file 2's, then the pairs; the lowest record of the first failing check raises BdxError naming the
    file, the 1-based record number, the byte offset of its first line in the plain text and the first broken rule
    (``_io="device-deal"``: the byte offset alone), after the batches before it were written; the failing batch is
    neither classified, counted nor written.  A paired run whose files hold different numbers of records raises BdxError
    after the last common batch is written instead of stopping silently at the shorter file.  A truncated last record
    fails the plus or the length rule.  Not checked: the sequence alphabet, the quality range, the headers behind
    their first blank.  ``_timings`` then also holds check_s and checked_records.
    Returns the DemuxStats scalar counters (the reference returns nothing)."""
    if not isinstance(_check, bool):
        raise ValueError("_check must be True or False")
    if len(args) == 3:
        fastq1, barcode_file, output_directory = args
        fastq2 = None
        paired = False
    elif len(args) == 4:
        fastq1, fastq2, barcode_file, output_directory = args
        paired = True
    else:
        raise TypeError("execute_demultiplexing takes 3 (single-end) or 4 (paired-end) positional arguments")
    if _gzip not in ("host", "device"):
        raise ValueError("_gzip must be 'host' or 'device'")
    if _gzip == "device" and _io not in ("device", "device-deal"):  # (no silent fallback to the host deflate)
        raise ValueError("_gzip='device' compresses inside the device FASTQ pipeline: it needs _io='device'")
    if isinstance(_gzip_level, bool) or _gzip_level not in (1, 2):
        raise ValueError("_gzip_level must be 1 or 2")
    if _gzip_level != 1 and _gzip != "device":  # (the host writers have one level)
        raise ValueError("_gzip_level selects a level of the device encoder: it needs _gzip='device'")
    if _gunzip not in ("host", "device", "device-stream", "device-window"):
        raise ValueError("_gunzip must be 'host', 'device', 'device-stream' or 'device-window'")
    if _gunzip != "host" and _io == "device-deal":  # (their text, or the state they carry, lives on one device)
        raise ValueError(f"_io='device-deal' takes a plain input or a .gz the host inflates: _gunzip must be 'host', not '{_gunzip}'")
    if _gunzip != "host" and _io != "device":  # (no silent fallback to the host inflate)
        raise ValueError(f"_gunzip='{_gunzip}' inflates inside the device FASTQ pipeline: it needs _io='device'")
    if _gunzip_window is not None:
        if _gunzip != "device-window":
            raise ValueError("_gunzip_window is the window of _gunzip='device-window'")
        _gunzip_window = deviceio.window_bytes(_gunzip_window)  # (ValueError: not an int of 1024 .. 2^28)
    if _span_bytes is not None:
        if _io != "device-deal":
            raise ValueError("_span_bytes is the span of _io='device-deal'")
        _span_bytes = deviceio.span_bytes(_span_bytes)  # (ValueError: not an int of at least 16)
    if _io == "device-deal":
        if paired:  # (the two files' spans do not hold the same record ranges)
            raise ValueError("_io='device-deal' takes single-end input: a second FASTQ file needs _io='device' or 'native'")
        if _classifier_factory is not None:  # (no silent fallback to the host pipeline)
            raise ValueError("_io='device-deal': the device FASTQ pipeline needs the HIP classifier (no _classifier_factory)")

    defaults = dict(
        barcode_file2=None, gzip_output=None, max_error_rate=0.2, min_delta=0.0, match=0, mismatch=1, indel=1,
        nindel=None, bc_complement=False, bc_rev=False, ref_search_range="1:end", barcode_start_range="1:end",
        barcode_end_range="1:end", ref_search_range2="1:end", barcode_start_range2="1:end",
        barcode_end_range2="1:end", chunk_size=4000, channel_capacity=64, trim_side=None, trim_side2=None,
        summary=False, summary_format="html", matching_algorithm="semiglobal", log=False)
    if paired:
        defaults.update(output_prefix1="", output_prefix2="", classify_both=False)
    else:
        defaults.update(output_prefix="")
    unknown = set(kw) - set(defaults)
    if unknown:
        raise TypeError(f"unsupported keyword argument(s): {sorted(unknown)}")
    o = {**defaults, **kw}
    devs = _device_list(device, devices, _io)
    multi = len(devs) > 1

    start_time = _dt.datetime.now()
    if o["log"]:  # core.jl:394-407 / :531-543
        _log("Info: BioDemuX demultiplexing started (MI355X HIP backend).")
        _log(f"  - Input 1: {os.path.basename(fastq1)}")
        if paired:
            _log(f"  - Input 2: {os.path.basename(fastq2)}")
        _log(f"  - Barcode File: {os.path.basename(barcode_file)}")
        _log(f"  - Output Directory: {output_directory}")
        _log(f"  - Max Error Rate: {o['max_error_rate']}")

    if _gunzip == "device":  # an input the device inflate cannot take: refused before the output directory is touched
        deviceio.check_gunzip_inputs([fastq1, fastq2] if paired else [fastq1], load_library())
    elif _gunzip in ("device-stream", "device-window"):  # ... or that is no gzip file at all
        deviceio.check_stream_inputs([fastq1, fastq2] if paired else [fastq1], _gunzip)

    if not os.path.isdir(output_directory):  # core.jl:410-412
        os.mkdir(output_directory)

    if paired:  # core.jl:414-419
        prefix1 = o["output_prefix1"] or _PREFIX_RE.sub("", os.path.basename(fastq1))
        prefix2 = o["output_prefix2"] or _PREFIX_RE.sub("", os.path.basename(fastq2))
        fastqs = [fastq1, fastq2]
        classify_both = o["classify_both"]
    else:  # core.jl:550-552
        prefix1 = o["output_prefix"] or _PREFIX_RE.sub("", os.path.basename(fastq1))
        prefix2 = ""
        fastqs = [fastq1]
        classify_both = False

    config = build_config(
        barcode_file, o["barcode_file2"], fastqs, o["gzip_output"], o["bc_complement"], o["bc_rev"], classify_both,
        float(o["max_error_rate"]), float(o["min_delta"]), o["match"], o["mismatch"], o["indel"], o["nindel"],
        o["ref_search_range"], o["barcode_start_range"], o["barcode_end_range"], o["ref_search_range2"],
        o["barcode_start_range2"], o["barcode_end_range2"], o["trim_side"], o["trim_side2"], o["summary"],
        o["summary_format"], o["matching_algorithm"])

    if _io == "device" and _classifier_factory is not None:  # (no silent fallback to the host pipeline)
        raise ValueError("_io='device': the device FASTQ pipeline needs the HIP classifier (no _classifier_factory)")
    # summary=true: the HIP classifier collects the histograms of classification.jl:827-865 on the device
    # (bdx_get_stats); a test-injected classifier without such tables hands over per-pass outputs instead
    classifiers = _open_classifiers(config, devs, _classifier_factory)
    if _timings is not None:  # barcode table + device context: before the first batch can move
        _timings["setup_s"] = (_dt.datetime.now() - start_time).total_seconds()
    device_stats = hasattr(classifiers[0], "stats_tables")
    hist = DemuxStats() if (config.summary and not device_stats) else None

    def on_batch(out):
        if hist is not None and "pass_bc" in out:
            hist.add_pass_outputs(out, float(config.min_delta))

    try:
        if _io not in ("auto", "native", "python", "device", "device-deal"):
            raise ValueError("_io must be 'auto', 'native', 'python' or 'device'")
        use_native = _io == "native" or (_io == "auto" and nativeio.available())
        if _timings is not None:
            _timings["pre_s"] = (_dt.datetime.now() - start_time).total_seconds()  # everything before the first batch can be read
        if _io == "device":
            deviceio.demux_device(fastq1, fastq2, config, output_directory, prefix1, prefix2, classifiers[0], _batch_reads,
                                  _timings, gzip_device=_gzip == "device", gzip_level=int(_gzip_level), gunzip=_gunzip,
                                  gunzip_window=_gunzip_window or deviceio.WINDOW_BYTES, check=_check)
        elif _io == "device-deal":
            deviceio.demux_device_dealt(fastq1, config, output_directory, prefix1, classifiers, _batch_reads, _timings,
                                        gzip_device=_gzip == "device", gzip_level=int(_gzip_level), span_bytes=_span_bytes,
                                        check=_check)
        elif use_native:
            t_call = _dt.datetime.now()
            nativeio.demux_native(fastq1, fastq2, config, output_directory, prefix1, prefix2, classifiers, _batch_reads,
                                  on_batch, _timings, check=_check)
            if _timings is not None:  # (beyond the pipeline's own wall clock: releasing its batch buffers)
                _timings["native_call_s"] = (_dt.datetime.now() - t_call).total_seconds()
        else:
            dealt: List[int] = []
            _demux(fastq1, fastq2, config, output_directory, prefix1, prefix2, classifiers, _batch_reads, on_batch,
                   dealt, check=_check, timings=_timings)
            if multi and _timings is not None:
                _timings["batches_per_device"] = dealt
        # merge_stats (reporting.jl:1-9) over the contexts: a host sum of a few KB, no collective
        counts = np.sum([np.asarray(c.counts, dtype=np.int64) for c in classifiers], axis=0)
        tables = (merge_stats_tables([c.stats_tables() for c in classifiers]) if (config.summary and device_stats)
                  else None)
        if (multi or _io == "device-deal") and _timings is not None:
            _timings["devices"] = list(devs)
    finally:
        t_close = _dt.datetime.now()
        _close_all(classifiers)
        if _timings is not None:  # releasing the device context (staging buffers, tables)
            _timings["close_s"] = (_dt.datetime.now() - t_close).total_seconds()

    duration = _dt.datetime.now() - start_time  # core.jl:484-485
    if _timings is not None:
        _timings["total_s"] = duration.total_seconds()
    if o["log"]:  # core.jl:487-491
        _log(f"Done: Finished in {canonical_duration(duration)}.")
    stats = DemuxStats.from_counts(counts, len(config.bc_seqs), len(config.bc_seqs2) if config.is_dual else 0)
    if tables is not None:
        stats.add_device_tables(tables, config)
    if hist is not None:
        for f in ("bc1", "bc2"):
            for k in ("pos_counts", "len_counts", "score_counts", "per_bc_score_counts", "per_bc_pos_counts",
                      "per_bc_len_counts"):
                setattr(stats, f"{f}_{k}", getattr(hist, f"{f}_{k}"))
    if config.summary:  # core.jl:493-497 / :626-630 (merge_stats over the workers: summed over the device contexts above)
        generate_summary_report(stats, config, output_directory, fastq1, barcode_file, fastq2, o["barcode_file2"],
                                bc_complement=o["bc_complement"], bc_rev=o["bc_rev"], trim_side=o["trim_side"],
                                trim_side2=o["trim_side2"], n_threads=1, duration=duration)
    return stats
