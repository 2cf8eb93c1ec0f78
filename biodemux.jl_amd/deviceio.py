"""Device FASTQ pipeline (``execute_demultiplexing(..., _io="device")``): FASTQ text goes to the GPU and per-output-file
FASTQ blocks come back.  Line index, packing, the stable split by output file (core.jl:139-148) and the gather of the
trimmed records (core.jl:162-173) run as kernels (csrc/bdx_fastq.hip, C-ABI bdx_fq_*_device); the host only copies
bytes and appends one block per file and batch (csrc/bdx_io.cpp bdx_fq_write_blocks).

Batches of ``batch_reads`` records flow through three overlapped stages:
  upload thread   byte window of batch k+1 from the input (pageable copies on a copy stream)
  calling thread  index -> pack -> classify -> gather of batch k on the context's stream, then the download of its blocks
  writer thread   waits for batch k-1's download and appends its blocks (one write per file, in batch order: per-file
                  order is input order)
Same files, bytes, counters and reports as nativeio.demux_native.

With ``gzip_device`` (``execute_demultiplexing(..., _gzip="device")``) and gzip output the calling thread also deflates
the batch's blocks on the device (csrc/bdx_deflate.hip, bdx_fq_deflate_level_device): only finished gzip members come back
and the writer appends them verbatim (bdx_fq_write_blocks_raw); the files then gunzip to the same bytes.

With ``gunzip="device"`` (``_gunzip="device"``: a _Members, not a _HostText) a ``.gz`` input that is a chain of size-tagged
gzip members (BGZF, or this library's own output) is not inflated on the host: the upload thread copies the COMPRESSED
members that cover the batch's byte window and the calling thread inflates them on the device right before the line
index (csrc/bdx_inflate.hip, bdx_fq_inflate_device, which checks every member's CRC-32 and ISIZE).  The cursor stays in
plain-text coordinates; the member at a batch's end is simply inflated again by the next batch.

With ``gunzip="device-stream"`` (``_gunzip="device-stream"``: a _ResidentText) a ``.gz`` input is an ORDINARY gzip file
(members of any size, no tags): before the first batch the whole compressed file is uploaded and inflated by
bdx_fq_inflate_stream_device (csrc/bdx_inflate_stream.hip: speculative block starts, every CRC-32 and ISIZE checked),
the compressed copy is freed and the text stays RESIDENT in device memory.  A batch's window is then a pointer into it:
nothing is uploaded per batch.  Peak device memory: the compressed bytes plus three times the plain bytes.

With ``gunzip="device-window"`` (``_gunzip="device-window"``: a _WindowedText) the same ordinary gzip file, of ANY
size, goes through the device in WINDOWS of ``gunzip_window`` compressed bytes (bdx_fq_inflate_window_*, csrc/
bdx_inflate_window_core.h): the upload thread copies the next window's compressed bytes while the calling thread works
on the current batch; the calling thread feeds a window, on the context's stream, whenever the text behind the cursor
is shorter than the batch wants; what a window left unconsumed (a block and a header at most, as a rule) is put in
front of the next one by a device-to-device copy; new text goes behind the text no batch has taken yet.  Peak device
memory of an input: two windows of compressed bytes (each with a reserve in front for the remainder), three times the
largest single window's text (the text and, during the call, its 16-bit image), and twice the text one batch holds —
whatever the file's size.  A window that holds no complete block is offered again twice as long, up to 2^28 bytes.
A member's CRC-32 and ISIZE are known at its end only: a refused member raises BdxError after the batches of the
windows before it were written, as with the host inflate; "refused before the first batch" holds for the resident
mode alone.

``execute_demultiplexing(..., _io="device-deal", devices=[...])`` is demux_device_dealt, at the end of this file: the same
device steps (_Context.batch) on several contexts.  The reference frames records by line count alone, so the text is cut
into byte spans, (newlines in front of a span) mod 4 tells which of its lines begin a record, and the spans' counts chain
with one addition each (_SpanChain); nothing waits for the index of the span before.  Single-end input, plain or
inflated by the host.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np

from . import checks, nativeio
from .hipabi import BdxError, pinned_empty
from .outputs import OutputLayout

_H2D, _D2H = 1, 2  # hipMemcpyKind
_NONBLOCKING = 1   # hipStreamNonBlocking
_NO_TIMING = 2     # hipEventDisableTiming


class _Runtime:
    """The few HIP runtime calls the pipeline makes, resolved through libbiodemux_hip.so (the runtime it links, so the
    device pointers and streams are the ones its C-ABI uses)."""

    def __init__(self, lib):
        vp = C.c_void_p
        sig = {
            "hipSetDevice": [C.c_int],
            "hipMalloc": [C.POINTER(vp), C.c_size_t],
            "hipFree": [vp],
            "hipMemcpyAsync": [vp, vp, C.c_size_t, C.c_int, vp],
            "hipStreamCreateWithFlags": [C.POINTER(vp), C.c_uint],
            "hipStreamDestroy": [vp],
            "hipStreamSynchronize": [vp],
            "hipEventCreateWithFlags": [C.POINTER(vp), C.c_uint],
            "hipEventRecord": [vp, vp],
            "hipEventSynchronize": [vp],
            "hipEventDestroy": [vp],
        }
        for name, args in sig.items():
            fn = getattr(lib, name)
            fn.restype = C.c_int
            fn.argtypes = args
            setattr(self, name, fn)
        lib.hipGetErrorString.restype = C.c_char_p
        lib.hipGetErrorString.argtypes = [C.c_int]
        self._err = lib.hipGetErrorString

    def check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise BdxError(f"{what} failed: {self._err(rc).decode()}")

    def stream(self) -> int:
        s = C.c_void_p()
        self.check(self.hipStreamCreateWithFlags(C.byref(s), _NONBLOCKING), "hipStreamCreateWithFlags")
        return s.value

    def event(self) -> int:
        e = C.c_void_p()
        self.check(self.hipEventCreateWithFlags(C.byref(e), _NO_TIMING), "hipEventCreateWithFlags")
        return e.value


class _DevBuf:
    def __init__(self, rt: _Runtime):
        self.rt, self.p, self.cap = rt, 0, 0

    def ensure(self, nbytes: int, exact: bool = False) -> int:
        if nbytes > self.cap:
            self.free()
            want = max(256, nbytes if exact else int(nbytes * 1.25))  # (room for the next batches' slightly longer windows)
            p = C.c_void_p()
            self.rt.check(self.rt.hipMalloc(C.byref(p), want), f"hipMalloc({want})")
            self.p, self.cap = p.value, want
        return self.p

    def free(self) -> None:
        if self.p:
            self.rt.hipFree(self.p)
        self.p, self.cap = 0, 0


_io_lib = None


def _io():
    """libbdx_io.so with the entries the device pipeline uses on top of nativeio's."""
    global _io_lib
    if _io_lib is None:
        L = nativeio._load()
        vp = C.c_void_p
        L.bdx_fq_data.restype = vp
        L.bdx_fq_data.argtypes = [vp]
        L.bdx_fq_wait.restype = C.c_int32
        L.bdx_fq_wait.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.bdx_fq_write_blocks.restype = C.c_int32
        L.bdx_fq_write_blocks.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
        L.bdx_fq_write_blocks_raw.restype = C.c_int32
        L.bdx_fq_write_blocks_raw.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
        _io_lib = L
    return _io_lib


def _is_gz(path: str) -> bool:
    return path.lower().endswith(".gz")  # fileio's rule (fileio.jl:78)


def open_members(path: str, lib) -> "nativeio.GzMembers":
    """The member table of a .gz input for the device inflate; ValueError (naming the file and the reason) when the file
    is not a chain of size-tagged members the device decoder takes — there is no silent fall-back to the host inflate."""
    g = nativeio.GzMembers(path, int(lib.bdx_fq_inflate_member_max()))
    if not g.eligible:
        why = g.reason
        g.close()
        raise ValueError(f"_gunzip='device' cannot take {path}: {why}; it inflates chains of size-tagged gzip members "
                         "(BGZF, or the output of _gzip='device') — use _gunzip='host'")
    return g


def check_gunzip_inputs(paths, lib) -> None:
    """execute_demultiplexing calls this before it makes the output directory: every .gz input must be eligible"""
    for p in paths:
        if _is_gz(p):
            open_members(p, lib).close()


def check_stream_inputs(paths, mode: str = "device-stream") -> None:
    """execute_demultiplexing calls this before it makes the output directory: a .gz input of the stream inflate
    (resident or windowed) begins with a gzip header"""
    for p in paths:
        if _is_gz(p):
            with open(p, "rb") as f:
                head = f.read(3)
            if head != b"\x1f\x8b\x08":
                raise ValueError(f"_gunzip='{mode}' cannot take {p}: it does not begin with a gzip header (1f 8b 08)")


STREAM_CHUNK = 0  # chunk_bytes of the stream inflate (0: bdx_fq_inflate_stream_chunk()); tools/e2e_device_probe.py sweeps it
_STREAM_INFO = ("stream_members", "stream_chunks", "stream_confirmed", "stream_discarded", "stream_no_candidate",
                "stream_longest_segment")
_E_SPACE = -5  # BDX_E_SPACE
# compressed bytes per window of _gunzip="device-window": the largest, and the fastest of 16, 64 and 256 MiB on the 10 M read
# file (a 16 MiB window costs some 0.14 s beyond its share of the inflate; profiles/r09_e2e_gunzip_window.json)
WINDOW_BYTES = 1 << 28
WINDOW_MIN, WINDOW_MAX = 1024, 1 << 28
_WINDOW_LEAD = 1 << 20  # room in front of a window's fresh bytes for what the window before left (or the window's size, if smaller)


def window_bytes(v) -> int:
    """_gunzip_window as execute_demultiplexing takes it: an int of 1024 .. 2^28 (ValueError otherwise)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not WINDOW_MIN <= int(v) <= WINDOW_MAX:
        raise ValueError(f"_gunzip_window must be an int of {WINDOW_MIN} .. {WINDOW_MAX} (2^28) compressed bytes, got {v!r}")
    return int(v)


def _add_stream_info(busy: dict, info) -> None:
    """the info words of one stream-inflate call onto the run's counters: sums, and the longest segment of all calls"""
    for name, v in zip(_STREAM_INFO, info.tolist()):
        busy[name] = max(v, busy.get(name, 0)) if name == "stream_longest_segment" else busy.get(name, 0) + v


def _upload_text(rt: _Runtime, L, f, s_copy: int, buf: _DevBuf, start: int, want: int, or_none: bool = False):
    """Bytes [start, start + want) of the host text ``f`` (mapped, or inflated so far by the host: waits for them), what
    is there of them -> the device buffer ``buf``.  -> (bytes, final); with ``or_none`` None, and no buffer, for no bytes"""
    avail, fin = C.c_int64(0), C.c_int32(0)
    if L.bdx_fq_wait(f.h, start + want, C.byref(avail), C.byref(fin)) != 0:
        raise OSError(L.bdx_io_last_error().decode())
    end = min(avail.value, start + want)
    nbytes = max(0, end - start)
    if or_none and not nbytes:
        return None
    dst = buf.ensure(nbytes + 64)
    if nbytes:
        rt.check(rt.hipMemcpyAsync(dst, L.bdx_fq_data(f.h) + start, nbytes, _H2D, s_copy), "hipMemcpyAsync (upload)")
        rt.check(rt.hipStreamSynchronize(s_copy), "hipStreamSynchronize (upload)")
    return nbytes, bool(fin.value) and end >= avail.value


class _Input:
    """One FASTQ input of demux_device: where it stands (``cursor``, in plain-text bytes), per window slot the text of a
    batch on the device (``win``: (bytes, final), ``d_text``: where it starts) and the line tables of the current batch.
    ``io_lib`` is libbdx_io.so, ``classifier`` the context the inflate and the index run on, ``busy`` the run's counters.
    How text gets into a slot is the subclass's business, in these hooks:
      prepare(s_main, s_copy)           the calling thread, once, before the first batch
      send(s_copy, slot, want)          the upload thread (through upload(), which counts upload_s)
      before_index(s_copy, slot, want)  the calling thread, in front of every line index
      widen(s_copy, slot, want)         the calling thread, after an index that came back short"""

    allowance = 65536  # what a window asks for beyond batch_reads average records
    inflates = False   # the run reports inflate_s, compressed_in_bytes and plain_in_bytes

    def __init__(self, path: str, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int):
        self.path, self.rt, self.L, self.cl, self.busy, self.batch_reads = path, rt, io_lib, classifier, busy, batch_reads
        self.cursor = 0
        self.avg_record = 330.0  # bytes per record, learned from the batches so far
        self.win = [(0, 0), (0, 0)]  # per window slot: (bytes, final)
        self.d_text = [0, 0]         # where the window's text starts on the device
        self.d_off, self.d_len = _DevBuf(rt), _DevBuf(rt)
        self.d_off.ensure(4 * batch_reads * 8)
        self.d_len.ensure(4 * batch_reads * 4)

    def want_bytes(self) -> int:
        return int(self.batch_reads * self.avg_record * 1.05) + self.allowance

    def upload(self, s_copy: int, slot: int, want: int):
        """bytes [cursor, cursor + want) of the input (what is there of them) -> the device window `slot`"""
        t0 = time.perf_counter()
        # (the current device belongs to the thread: the upload thread has to choose it as well)
        self.rt.check(self.rt.hipSetDevice(int(getattr(self.cl, "device", 0))), "hipSetDevice")
        self.send(s_copy, slot, want)
        self.busy["upload_s"] += time.perf_counter() - t0

    def index(self, s_copy: int, slot: int):
        """The line table of the batch that starts window `slot` (on the context's stream, after the inflate if there is one)
        -> (records, bytes they take).  A window that ends before ``batch_reads`` records do is widened to twice its size."""
        want = self.want_bytes()
        while True:
            self.before_index(s_copy, slot, want)
            nbytes, final = self.win[slot]
            n, nxt = C.c_int64(0), C.c_int64(0)
            self.cl._check(self.cl.lib.bdx_fq_index_device(self.cl.h, self.d_text[slot], nbytes, int(final), self.batch_reads,
                                                           self.d_off.p, self.d_len.p, C.byref(n), C.byref(nxt)))
            if n.value >= self.batch_reads or final:
                return n.value, nxt.value
            want = 2 * max(want, nbytes)  # a record did not fit: a larger window
            self.widen(s_copy, slot, want)

    def prepare(self, s_main: int, s_copy: int):
        pass

    def before_index(self, s_copy: int, slot: int, want: int):
        pass

    def widen(self, s_copy: int, slot: int, want: int):
        t_up = time.perf_counter()
        self.upload(s_copy, slot, want)
        self.busy["device_s"] -= time.perf_counter() - t_up  # (upload_s has it; the driver counts the whole index() call)

    def release(self):
        """everything below the cursor is uploaded: the host pages can go"""

    def free(self, *bufs: _DevBuf):  # the line tables and the subclass's device buffers: from its close()
        for b in (*bufs, self.d_off, self.d_len):
            b.free()


class _HostText(_Input):
    """a plain input, or a .gz the host inflates in the background: the text's bytes go up, two device buffers of them"""

    def __init__(self, path: str, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int):
        self.f, self.text = nativeio.FastqFile(path), [_DevBuf(rt), _DevBuf(rt)]
        super().__init__(path, rt, io_lib, classifier, busy, batch_reads)

    def send(self, s_copy: int, slot: int, want: int):
        self.win[slot] = _upload_text(self.rt, self.L, self.f, s_copy, self.text[slot], self.cursor, want)
        self.d_text[slot] = self.text[slot].p

    def release(self):
        self.f.release(self.cursor)

    def close(self):
        self.free(*self.text)
        self.f.close()


class _Members(_Input):
    """_gunzip="device": the mapped COMPRESSED members and their table; per slot those of the window and their text"""

    inflates = True

    def __init__(self, path: str, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int, members):
        self.gz, self.wmem = members, [(0, 0), (0, 0)]  # the table, and the members of a slot: [first, last)
        self.comp, self.text = [_DevBuf(rt), _DevBuf(rt)], [_DevBuf(rt), _DevBuf(rt)]
        super().__init__(path, rt, io_lib, classifier, busy, batch_reads)

    def send(self, s_copy: int, slot: int, want: int):
        """the compressed members that cover the text bytes [cursor, cursor + want) -> the device buffer comp[slot]"""
        g, rt = self.gz, self.rt
        n, po = len(g), g.plain_off
        m0 = min(int(np.searchsorted(po, self.cursor, side="right")) - 1, n)  # the member that holds the cursor
        m1 = max(m0, min(int(np.searchsorted(po, self.cursor + want, side="left")), n))
        while m1 < n and g.isize[m1] == 0:  # (an empty member behind the window: the BGZF end marker)
            m1 += 1
        if m1 > m0:
            c0 = int(g.comp_off[m0])
            nbytes = int(g.comp_off[m1 - 1]) + int(g.comp_len[m1 - 1]) - c0
            dst = self.comp[slot].ensure(nbytes)
            rt.check(rt.hipMemcpyAsync(dst, g.data + c0, nbytes, _H2D, s_copy), "hipMemcpyAsync (upload)")
            rt.check(rt.hipStreamSynchronize(s_copy), "hipStreamSynchronize (upload)")
            self.busy["compressed_in_bytes"] += nbytes
        self.wmem[slot] = (m0, m1)
        self.win[slot] = (max(0, int(po[m1]) - self.cursor), m1 == n)

    def before_index(self, s_copy: int, slot: int, want: int):
        """comp[slot] -> text[slot] on the context's stream; the window's text starts at the cursor, somewhere inside
        the first member"""
        t_i = time.perf_counter()
        g, lib, h = self.gz, self.cl.lib, self.cl.h
        m0, m1 = self.wmem[slot]
        k = m1 - m0
        total = int(g.plain_off[m1] - g.plain_off[m0])
        d_text = self.text[slot].ensure(total + 64)
        if k:
            coff = np.ascontiguousarray(g.comp_off[m0:m1] - g.comp_off[m0])
            poff = np.ascontiguousarray(g.plain_off[m0:m1] - g.plain_off[m0])
            clen = np.ascontiguousarray(g.comp_len[m0:m1])
            plen = np.ascontiguousarray(g.isize[m0:m1])
            status = np.zeros(k, dtype=np.int32)
            rc = lib.bdx_fq_inflate_device(h, self.comp[slot].p, coff.ctypes.data, clen.ctypes.data, poff.ctypes.data,
                                           plen.ctypes.data, k, d_text, total, status.ctypes.data)
            if rc != 0:
                bad = np.flatnonzero(status)
                msg = lib.bdx_last_error(h).decode()
                if len(bad):
                    msg = f"{self.path}: gzip member {m0 + int(bad[0])} is refused by the device inflate ({msg})"
                raise BdxError(msg)
            self.busy["plain_in_bytes"] += total
        self.d_text[slot] = d_text + (self.cursor - int(g.plain_off[m0]))
        self.busy["inflate_s"] += time.perf_counter() - t_i

    def release(self):
        if len(self.gz):
            m = min(int(np.searchsorted(self.gz.plain_off, self.cursor, side="right")) - 1, len(self.gz) - 1)
            self.gz.release(int(self.gz.comp_off[m]))

    def close(self):
        self.free(*self.text, *self.comp)
        self.gz.close()


class _ResidentText(_Input):
    """_gunzip="device-stream": the stream inflate puts the whole text into device memory once; a window is a place in it"""

    inflates = True

    def __init__(self, path: str, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int):
        self.res, self.res_len = _DevBuf(rt), 0  # the resident text and its length
        super().__init__(path, rt, io_lib, classifier, busy, batch_reads)

    def prepare(self, s_main: int, s_copy: int):
        """The whole .gz file -> the resident text, on the context's stream: the compressed bytes go up,
        bdx_fq_inflate_stream_device is called with a guessed capacity and once more with the exact one when that was
        too small, the compressed copy is freed."""
        rt, lib, h = self.rt, self.cl.lib, self.cl.h
        g = nativeio.GzMembers(self.path, int(lib.bdx_fq_inflate_member_max()))  # (maps any .gz; its table is not used)
        comp = _DevBuf(rt)
        try:
            size = int(g.size)
            plen, info = C.c_int64(0), np.zeros(8, dtype=np.int64)
            t_u = time.perf_counter()
            try:
                comp.ensure(size, exact=True)
                if size:
                    rt.check(rt.hipMemcpyAsync(comp.p, g.data, size, _H2D, s_copy), "hipMemcpyAsync (upload)")
                    rt.check(rt.hipStreamSynchronize(s_copy), "hipStreamSynchronize (upload)")
                self.busy["upload_s"] += time.perf_counter() - t_u
                t_i = time.perf_counter()
                cap = 4 * size  # FASTQ deflates 3 .. 5 x: usually one call
                for _ in range(2):
                    self.res.free()
                    self.res.ensure(cap + 64, exact=True)
                    rc = lib.bdx_fq_inflate_stream_device(h, comp.p, size, int(STREAM_CHUNK), self.res.p, cap, C.byref(plen),
                                                          info.ctypes.data)
                    if rc != _E_SPACE:
                        break
                    cap = int(plen.value)
            except BdxError as e:  # (an allocation of this module)
                raise BdxError(f"{self.path}: the stream inflate keeps the compressed bytes ({size}) and three times the plain "
                               f"bytes ({int(plen.value) or 'not known yet'}) in device memory: {e}") from None
            if rc == -2:  # BDX_E_DEVICE: the staging image (twice the plain bytes) did not fit
                raise BdxError(f"{self.path}: the stream inflate needs {size} compressed + 3 x {int(plen.value)} plain bytes of device "
                               f"memory ({lib.bdx_last_error(h).decode()})")
            if rc != 0:
                raise BdxError(f"{self.path}: refused by the device stream inflate: {lib.bdx_last_error(h).decode()}")
            self.res_len = int(plen.value)
            self.busy["compressed_in_bytes"] += size
            self.busy["plain_in_bytes"] += self.res_len
            _add_stream_info(self.busy, info)
            self.busy["inflate_s"] += time.perf_counter() - t_i
        finally:
            comp.free()
            g.close()

    def send(self, s_copy: int, slot: int, want: int):
        end = min(self.res_len, self.cursor + want)  # (64 bytes of slack follow the text's end)
        self.win[slot] = (max(0, end - self.cursor), end >= self.res_len)
        self.d_text[slot] = self.res.p + self.cursor

    def close(self):
        self.free(self.res)


class _WindowedText(_Input):
    """_gunzip="device-window": the file is mapped, its text appears in ``res`` a window of ``window`` compressed bytes at
    a time (feed) and leaves it batch by batch.  The upload thread brings the next window's compressed bytes (fetch);
    the calling thread feeds windows in front of every index until the batch has its text."""

    allowance = 4096  # (what it asks for stays in device memory: a small allowance; index() doubles it when it was short)
    inflates = True

    def __init__(self, path: str, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int, window: int):
        lib, h = classifier.lib, classifier.h
        chunk = int(STREAM_CHUNK) or int(lib.bdx_fq_inflate_stream_chunk())
        self.wbytes = min(WINDOW_MAX, -(-window // chunk) * chunk)  # a multiple of the chunk size
        self.lead = min(self.wbytes, _WINDOW_LEAD)
        self.wmap = nativeio.GzMembers(path, int(lib.bdx_fq_inflate_member_max()))  # (maps any .gz; its table is not used)
        self.wsize = int(self.wmap.size)
        self.w = C.c_void_p()  # the window object
        try:
            classifier._check(lib.bdx_fq_inflate_window_open(h, int(STREAM_CHUNK), C.byref(self.w)))
        except BaseException:
            self.wmap.close()
            raise
        self.res = _DevBuf(rt)  # the text no batch has taken yet: res_len bytes from the plain offset t_base
        self.res_len = self.t_base = 0
        self.comp = [_DevBuf(rt), _DevBuf(rt)]  # two windows of compressed bytes
        self.s_main = 0      # the context's stream (prepare)
        self.f_up = 0        # the file's bytes below it have gone up
        self.pos = 0         # where the window object stands: the sum of what it consumed
        self.released = 0    # the host pages below it were let go
        self.pending = None  # the window that went up and was not fed yet: [buffer, first byte, end, offset in the buffer]
        self.cur = None      # the window fed last, likewise: the file's bytes [pos, end) of it are the remainder
        self.ended = False   # the last window is through
        self.ratio = 4.5     # plain bytes per compressed byte, learned from the windows so far
        busy.setdefault("stream_windows", 0)
        busy["stream_window_bytes"] = self.wbytes
        busy.setdefault("stream_text_peak_bytes", 0)
        super().__init__(path, rt, io_lib, classifier, busy, batch_reads)

    def prepare(self, s_main: int, s_copy: int):
        self.s_main = s_main

    def send(self, s_copy: int, slot: int, want: int):
        """the next window's compressed bytes, beside the current batch's kernels"""
        if self.pending is None and self.f_up < self.wsize:
            self.fetch(s_copy, self.wbytes)

    def fetch(self, s_copy: int, n: int):
        """the file's next n bytes (what is there of them) -> the device buffer the current window is not in, behind
        its reserve (the upload thread; the calling thread when it needs a window at once)"""
        rt = self.rt
        i = 1 - self.cur[0] if self.cur is not None else 0
        n = min(n, self.wsize - self.f_up, WINDOW_MAX - self.lead)  # (with the remainder in front still a window the entry takes)
        dst = self.comp[i].ensure(self.lead + n, exact=True)
        if n:
            rt.check(rt.hipMemcpyAsync(dst + self.lead, self.wmap.data + self.f_up, n, _H2D, s_copy), "hipMemcpyAsync (upload)")
            rt.check(rt.hipStreamSynchronize(s_copy), "hipStreamSynchronize (upload)")
        self.pending = [i, self.f_up, self.f_up + n, self.lead]
        self.f_up += n
        self.busy["compressed_in_bytes"] += n

    def _d2d(self, dst: int, src: int, n: int):
        if n:
            self.rt.check(self.rt.hipMemcpyAsync(dst, src, n, 3, self.s_main), "hipMemcpyAsync (device to device)")

    def feed(self, s_copy: int, grow: int = 0):
        """One more window through the window object, on the context's stream: the remainder of the window before goes
        in front of the pending one (fetched here when the upload thread has not brought one; `grow`: at least that
        many fresh bytes, after a window without progress), the text behind the text no batch has taken yet.
        -> True when the object made progress"""
        rt, lib = self.rt, self.cl.lib
        t_i = time.perf_counter()
        if self.pending is None:
            t_u = time.perf_counter()
            self.fetch(s_copy, max(grow, self.wbytes))
            self.busy["upload_s"] += time.perf_counter() - t_u
            t_i += time.perf_counter() - t_u
        nxt, self.pending = self.pending, None
        if self.cur is not None:
            i, f0, f1, off = self.cur
            rem = f1 - self.pos
            src = self.comp[i].p + off + (self.pos - f0)
            if rem > nxt[3]:  # more than the reserve holds: a buffer for both, nothing goes up again
                both = _DevBuf(rt)
                both.ensure(rem + (nxt[2] - nxt[1]) + 64, exact=True)
                self._d2d(both.p, src, rem)
                self._d2d(both.p + rem, self.comp[nxt[0]].p + nxt[3], nxt[2] - nxt[1])
                rt.check(rt.hipStreamSynchronize(self.s_main), "hipStreamSynchronize")
                self.comp[nxt[0]].free()
                self.comp[nxt[0]] = both
                nxt[3] = rem
            else:
                self._d2d(self.comp[nxt[0]].p + nxt[3] - rem, src, rem)
            nxt[1], nxt[3] = self.pos, nxt[3] - rem
        self.cur = nxt
        i, f0, f1, off = nxt
        flen = min(f1 - f0, WINDOW_MAX)
        last = int(f0 + flen == self.wsize)
        used, plen, info = C.c_int64(0), C.c_int64(0), np.zeros(8, dtype=np.int64)
        need = int(flen * self.ratio * 1.1) + 4096
        for attempt in range(2):
            self.text_room(need)
            room = self.res.cap - self.res_len - 64
            rc = lib.bdx_fq_inflate_window_feed(self.w, self.comp[i].p + off, flen, last, self.res.p + self.res_len, room, C.byref(used),
                                                C.byref(plen), info.ctypes.data)
            if rc != _E_SPACE:
                break
            need = int(plen.value)  # the room it asked for: the same call again, once
        if rc != 0:
            raise BdxError(f"{self.path}: refused by the device stream inflate in the window at compressed byte {self.pos}: "
                           f"{lib.bdx_last_error(self.cl.h).decode()}")
        self.pos += int(used.value)
        self.res_len += int(plen.value)
        self.ended = bool(last)
        if plen.value and flen:
            self.ratio = max(1.0, plen.value / max(1, used.value))
        self.busy["plain_in_bytes"] += int(plen.value)
        self.busy["stream_windows"] += 1
        _add_stream_info(self.busy, info)
        self.busy["inflate_s"] += time.perf_counter() - t_i
        return bool(used.value or plen.value or last)

    def text_room(self, need: int):
        """room for `need` more bytes of text (and 64 of slack) behind res_len: the text no batch has taken yet moves to
        the front when it does not overlap itself there, else into a larger buffer.  On the context's stream: ordered
        behind the gathers of the batch before, which read the old places."""
        keep = self.t_base + self.res_len - self.cursor
        front = self.cursor - self.t_base
        if self.res.cap - self.res_len - 64 >= need:
            return
        if front >= keep and self.res.cap - keep - 64 >= need:
            self._d2d(self.res.p, self.res.p + front, keep)
        else:
            new = _DevBuf(self.rt)
            new.ensure(keep + need + 64, exact=True)
            self._d2d(new.p, self.res.p + front, keep)
            self.rt.check(self.rt.hipStreamSynchronize(self.s_main), "hipStreamSynchronize")
            self.res.free()
            self.res = new
            self.busy["stream_text_peak_bytes"] = max(self.busy["stream_text_peak_bytes"], new.cap)
        self.t_base, self.res_len = self.cursor, keep

    def before_index(self, s_copy: int, slot: int, want: int):
        """fill: windows until `want` bytes of text lie behind the cursor or the file has ended -> the batch's window"""
        grow = 0
        while not self.ended and self.t_base + self.res_len - self.cursor < want:
            if self.feed(s_copy, grow):
                grow = 0
                continue
            have = self.cur[2] - self.pos  # no progress: no complete block in it — twice as long, to the file's end
            if have >= WINDOW_MAX or (self.cur[2] >= self.wsize):
                raise BdxError(f"{self.path}: a deflate block at compressed byte {self.pos} does not fit a window of {WINDOW_MAX} bytes")
            grow = min(max(have, self.wbytes), WINDOW_MAX - have)
        avail = self.t_base + self.res_len - self.cursor
        nbytes = min(avail, want)
        self.win[slot] = (nbytes, self.ended and avail <= want)
        self.d_text[slot] = self.res.p + (self.cursor - self.t_base)

    def widen(self, s_copy: int, slot: int, want: int):
        pass  # (before_index feeds again: nothing goes up a second time)

    def release(self):
        if self.pos > self.released:  # (once a window, not once a batch: dropping pages the runtime may still have pinned is not free)
            self.wmap.release(self.pos)
            self.released = self.pos

    def close(self):
        self.free(*self.comp, self.res)
        self.cl.lib.bdx_fq_inflate_window_close(self.w)
        self.wmap.close()


def _open_input(path: str, gunzip: str, window: int, rt: _Runtime, io_lib, classifier, busy: dict, batch_reads: int) -> _Input:
    """the _Input of ``path`` under ``gunzip`` (the values of _gunzip); a plain input is host text under every one"""
    args = (path, rt, io_lib, classifier, busy, batch_reads)
    if gunzip == "host" or not _is_gz(path):
        return _HostText(*args)
    if gunzip == "device":
        members = open_members(path, classifier.lib)
        try:
            return _Members(*args, members)
        except BaseException:
            members.close()
            raise
    return _ResidentText(*args) if gunzip == "device-stream" else _WindowedText(*args, int(window))


def _fetch(rt: _Runtime, stream: int, d_ptr: int, dtype, count: int) -> np.ndarray:
    """a small download: ``count`` items of ``dtype`` at the device address ``d_ptr`` (waits for ``stream``)"""
    out = np.zeros(max(count, 1), dtype=dtype)
    if count:
        rt.check(rt.hipMemcpyAsync(out.ctypes.data, d_ptr, count * out.itemsize, _D2H, stream), "hipMemcpyAsync (download)")
    rt.check(rt.hipStreamSynchronize(stream), "hipStreamSynchronize")
    return out[:count]


def _check_records(rt: _Runtime, cl, stream: int, path: str, text, n: int, base: int, done, busy: dict):
    """_check: the n records of one input's batch against the three record rules (bdx_fq_check_device on the context's
    stream).  ``text``: (d_text, bytes, d_off, d_len); ``base``: the window's offset in the plain text; ``done``: the
    records in front of the batch, None where only byte offsets are known.  -> the BdxError of the lowest record that
    breaks a rule (its line lengths come by a small download), or None"""
    d_text, nbytes, d_off, d_len = text
    bad, broken = C.c_int64(-1), C.c_int32(0)
    cl._check(cl.lib.bdx_fq_check_device(cl.h, d_text, nbytes, d_off, d_len, n, checks.ALL_RULES, C.byref(bad), C.byref(broken)))
    busy["checked_records"] += n
    if bad.value < 0:
        return None
    i = int(bad.value)
    off = _fetch(rt, stream, d_off + 4 * i * 8, np.int64, 4)
    ln = _fetch(rt, stream, d_len + 4 * i * 4, np.int32, 4)
    return checks.record_error(path, None if done is None else done + i + 1, base + int(off[0]), int(broken.value), int(ln[1]), int(ln[3]))


def _check_pairs(rt: _Runtime, cl, stream: int, paths, texts, n: int, done: int):
    """_check: the read names of the n record pairs of a batch (bdx_fq_check_pair_device) -> the BdxError of the lowest
    pair whose names differ (the two header lines come by a small download), or None"""
    (t1, b1, o1, l1), (t2, b2, o2, l2) = texts
    bad = C.c_int64(-1)
    cl._check(cl.lib.bdx_fq_check_pair_device(cl.h, t1, b1, o1, l1, t2, b2, o2, l2, n, C.byref(bad)))
    if bad.value < 0:
        return None
    i, heads = int(bad.value), []
    for d_text, _, d_off, d_len in texts:
        off = int(_fetch(rt, stream, d_off + 4 * i * 8, np.int64, 1)[0])
        ln = int(_fetch(rt, stream, d_len + 4 * i * 4, np.int32, 1)[0])
        heads.append(_fetch(rt, stream, d_text + off, np.uint8, ln).tobytes())
    return checks.pair_error(*paths, done + i + 1, *heads)


class _Slots:
    """The pinned download buffers: batch k is downloaded into one while the writer appends batch k - 1 from the other.
    ``free`` holds the slots the writer is done with, ``events[s]`` fires when the copy into ``hbuf[s]`` has landed."""

    def __init__(self, rt: _Runtime, n: int = 2):
        self.events = [rt.event() for _ in range(n)]
        self.hbuf = [None] * n
        self.free: "queue.Queue" = queue.Queue()
        for s in range(n):
            self.free.put(s)


class _Context:
    """One device context's share of a pipeline: its two streams, the pinned download slots, the result buffers of a
    batch, and the batch step itself.  ``busy`` takes device_s, batches and, with ``dev_gz``, the deflate's counters;
    ``errors`` is the run's list: a download that waits for a slot gives up once it has an entry."""

    def __init__(self, rt: _Runtime, classifier, busy: dict, layout: OutputLayout, dev_gz: bool, gzip_level: int, errors: list):
        self.rt, self.cl, self.busy, self.layout, self.dev_gz, self.errors = rt, classifier, busy, layout, dev_gz, errors
        if dev_gz:
            busy.update(deflate_s=0.0, plain_bytes=0, compressed_bytes=0, gzip_level=int(gzip_level))
        self.s_main, self.s_copy, self.slots = 0, 0, None
        self.seq, self.seq_off, self.out, self.gz = (_DevBuf(rt) for _ in range(4))
        self.v = {k: _DevBuf(rt) for k in ("bc1", "bc2", "keep_start", "keep_end")}

    def open(self):
        rt = self.rt
        rt.check(rt.hipSetDevice(int(getattr(self.cl, "device", 0))), "hipSetDevice")
        self.s_main, self.s_copy = rt.stream(), rt.stream()
        self.cl.set_stream(self.s_main)
        self.slots = _Slots(rt)

    def size_results(self, n: int):
        """room for the results of n records (each pipeline sizes them its own way: once a run, or once a span)"""
        self.seq_off.ensure((n + 1) * 8)
        for b in self.v.values():
            b.ensure(n * 4)

    def batch(self, texts, n: int, t0: float):
        """The n records of a batch: pack (the first input's reads) -> ONE classify call -> a gather per output stream ->
        with ``dev_gz`` the deflate (only finished gzip members come back) -> the start of the download.  ``texts``: per input
        its window and line tables, (d_text, bytes, d_off, d_len); ``t0``: where the batch's device_s began.  -> (slot, blocks)"""
        cl, lib, layout, v = self.cl, self.cl.lib, self.layout, self.v
        d_text, nbytes, d_off, d_len = texts[0]
        self.seq.ensure(nbytes + 64)
        cl._check(lib.bdx_fq_pack_device(cl.h, d_text, nbytes, d_off, d_len, n, self.seq.p, self.seq.cap, self.seq_off.p, None))
        cl.classify_device(self.seq.p, self.seq_off.p, n, **{k: b.p for k, b in v.items()})
        self.out.ensure(sum(texts[i][1] + 64 for i, _, _ in layout.streams))
        blocks, pos = [], 0
        for i, prefix, trim in layout.streams:
            d_text, nbytes, d_off, d_len = texts[i]
            cb = np.zeros(layout.n_classes, dtype=np.int64)
            cl._check(lib.bdx_fq_gather_device(cl.h, d_text, nbytes, d_off, d_len, n, v["bc1"].p, v["bc2"].p, layout.stride,
                                               layout.n_classes, v["keep_start"].p, v["keep_end"].p, int(bool(trim)),
                                               self.out.p + pos, self.out.cap - pos, cb.ctypes.data))
            blocks.append((pos, cb, prefix))
            pos += int(cb.sum())
        d_src = self.out
        if self.dev_gz:
            blocks, pos = self.deflate(blocks)
            d_src = self.gz
        self.busy["device_s"] += time.perf_counter() - t0
        self.busy["batches"] += 1
        return self.download(d_src, pos), blocks

    def deflate(self, blocks):
        """The batch's gathered blocks in ``out`` (the streams' blocks are one run of n_classes * len(blocks) blocks: one
        deflate call, at the level in busy["gzip_level"]) -> finished gzip members in ``gz``; -> (their blocks, their bytes)"""
        t_z = time.perf_counter()
        cl, lib, busy, n_classes = self.cl, self.cl.lib, self.busy, self.layout.n_classes
        cb_all = np.concatenate([cb for _, cb, _ in blocks])
        self.gz.ensure(int(lib.bdx_fq_deflate_bound(cb_all.ctypes.data, len(cb_all))))
        zb = np.zeros(len(cb_all), dtype=np.int64)
        cl._check(lib.bdx_fq_deflate_level_device(cl.h, busy["gzip_level"], self.out.p, cb_all.ctypes.data, len(cb_all), self.gz.p,
                                                  self.gz.cap, zb.ctypes.data))
        busy["plain_bytes"] += int(cb_all.sum())
        zblocks, pos = [], 0
        for k, (_, _, prefix) in enumerate(blocks):
            cz = zb[k * n_classes:(k + 1) * n_classes].copy()
            zblocks.append((pos, cz, prefix))
            pos += int(cz.sum())
        busy["compressed_bytes"] += pos
        busy["deflate_s"] += time.perf_counter() - t_z
        return zblocks, pos

    def download(self, d_src: _DevBuf, nbytes: int):
        """Starts the copy of the batch's `nbytes` into a free host slot (the writer hands them back) and records the
        slot's event behind it: the writer waits for the copy.  -> the slot, or None when the run has failed meanwhile"""
        rt, slots = self.rt, self.slots
        while True:
            try:
                hs = slots.free.get(timeout=0.05)
                break
            except queue.Empty:
                if self.errors:
                    return None
        if self.errors:
            return None
        if slots.hbuf[hs] is None or len(slots.hbuf[hs]) < nbytes:
            slots.hbuf[hs] = pinned_empty(max(nbytes, 1) + (max(nbytes, 1) >> 3), np.uint8)
        if nbytes:
            rt.check(rt.hipMemcpyAsync(slots.hbuf[hs].ctypes.data, d_src.p, nbytes, _D2H, self.s_main), "hipMemcpyAsync (download)")
        rt.check(rt.hipEventRecord(slots.events[hs], self.s_main), "hipEventRecord")
        return hs

    def close(self):
        rt = self.rt
        rt.hipSetDevice(int(getattr(self.cl, "device", 0)))
        if self.s_main:
            rt.hipStreamSynchronize(self.s_main)
            self.cl.set_stream(None)
        for b in (self.seq, self.seq_off, self.out, self.gz, *self.v.values()):
            b.free()
        for e in (self.slots.events if self.slots is not None else ()):
            rt.hipEventDestroy(e)
        for s in filter(None, (self.s_main, self.s_copy)):
            rt.hipStreamDestroy(s)


def _write_blocks(rt: _Runtime, L, layout: OutputLayout, raw: bool, T: int, busy: dict, slots: _Slots, slot: int, blocks):
    """What a writer thread does with one batch: waits for its download into ``slots.hbuf[slot]``, appends one block per
    file and stream, and hands the slot back.  ``raw``: the blocks are finished gzip members, appended as they are."""
    try:
        t0 = time.perf_counter()
        rt.check(rt.hipEventSynchronize(slots.events[slot]), "hipEventSynchronize (download)")
        t1 = time.perf_counter()
        base = slots.hbuf[slot].ctypes.data
        for off, cb, prefix in blocks:
            paths = layout.c_paths(prefix, np.flatnonzero(cb))
            if raw:
                rc = L.bdx_fq_write_blocks_raw(base + off, cb.ctypes.data, layout.n_classes, paths, T)
            else:
                rc = L.bdx_fq_write_blocks(base + off, cb.ctypes.data, layout.n_classes, paths, layout.gz, T)
            if rc != 0:
                raise OSError(L.bdx_io_last_error().decode())
        busy["download_s"] += t1 - t0
        busy["write_s"] += time.perf_counter() - t1
    finally:
        slots.free.put(slot)


def _write_loop(q_w, slots: _Slots, errors: list, *writer):
    """The writer thread: the batches in queue order (``writer``: _write_blocks' first arguments), until the run fails"""
    for slot, blocks in iter(q_w.get, None):
        if errors:
            slots.free.put(slot)
            continue
        try:
            _write_blocks(*writer, slots, slot, blocks)
        except BaseException as e:  # noqa: BLE001 - forwarded to the caller
            errors.append(e)


def demux_device(fastq1: str, fastq2: Optional[str], config, output_directory: str, prefix1: str, prefix2: str,
                 classifier, batch_reads: int, timings: Optional[dict] = None, gzip_device: bool = False,
                 gzip_level: int = 1, gunzip: str = "host", gunzip_window: int = WINDOW_BYTES, check: bool = False) -> None:
    """Device counterpart of nativeio.demux_native (same arguments but ``on_batch``: the HIP classifier keeps the
    summary tables itself).  ``classifier`` must be the HIP classifier.  ``gzip_device``: gzip output is compressed by
    bdx_fq_deflate_device after the gathers, only finished gzip members are downloaded and the writer appends them as
    they are (inert when the output is not gzip), at ``gzip_level`` (1 or 2: bdx_fq_deflate_level_device).
    ``gunzip`` (the values of _gunzip) says who inflates an input whose name ends in .gz, each such input on its own
    (inert for a plain input), ``gunzip_window`` how many compressed bytes a window of "device-window" has: _open_input
    picks the class, the module docstring has each one's flow, memory bound and what it refuses, and when.
    ``check`` (_check): after the line index of a batch and before its cursors move, every input's records are held to
    the record rules and a paired batch to the pair rule (bdx_fq_check_device, bdx_fq_check_pair_device); at the first
    failure the loop ends as at the input's end — the writer appends what it holds — and the BdxError is raised then.
    Two files of a pair with different numbers of records are refused likewise, behind the last common batch.
    timings then also holds check_s (a part of device_s) and checked_records."""
    if not hasattr(classifier, "classify_device"):
        raise ValueError("the device FASTQ pipeline (_io='device') needs the HIP classifier")
    t_wall = time.perf_counter()
    busy = {"upload_s": 0.0, "device_s": 0.0, "download_s": 0.0, "write_s": 0.0, "batches": 0}
    L = _io()
    rt = _Runtime(classifier.lib)
    rt.check(rt.hipSetDevice(int(getattr(classifier, "device", 0))), "hipSetDevice")
    T = nativeio._threads()
    batch_reads = max(1, int(batch_reads))
    paired = fastq2 is not None
    layout = OutputLayout(config, output_directory, prefix1, prefix2, paired)
    dev_gz = bool(gzip_device) and bool(layout.gz)
    ins, errors = [], []
    ctx = _Context(rt, classifier, busy, layout, dev_gz, gzip_level, errors)
    q_w: "queue.Queue" = queue.Queue(maxsize=1)
    up = ThreadPoolExecutor(max_workers=1, thread_name_prefix="bdx-upload")
    fut = writer = None
    refused = None  # (_check) a failed check: raised once the writer has appended every batch in front of it
    done = 0        # records of the batches so far
    if check:
        busy.update(check_s=0.0, checked_records=0)
    try:
        for path in (fastq1, fastq2) if paired else (fastq1,):  # (each input judged on its own)
            ins.append(_open_input(path, gunzip, gunzip_window, rt, L, classifier, busy, batch_reads))
        if any(inp.inflates for inp in ins):
            busy.update(inflate_s=0.0, compressed_in_bytes=0, plain_in_bytes=0)
        ctx.open()
        for inp in ins:
            inp.prepare(ctx.s_main, ctx.s_copy)
        ctx.size_results(batch_reads)

        def upload_all(slot: int):
            for inp in ins:
                inp.upload(ctx.s_copy, slot, inp.want_bytes())

        writer = threading.Thread(target=_write_loop, name="bdx-device-writer",
                                  args=(q_w, ctx.slots, errors, rt, L, layout, dev_gz, T, busy))
        writer.start()
        slot = 0
        fut = up.submit(upload_all, slot)
        while True:
            fut.result()  # 1. the upload of this batch's windows
            fut = None
            if errors:
                break
            t0 = time.perf_counter()
            found = [inp.index(ctx.s_copy, slot) for inp in ins]  # 2. the line index of each input
            ns = [k for k, _ in found]
            n = min(ns)
            last = paired and ns[0] != ns[1]  # lock-step pairs: stop at the shorter file (core.jl:48)
            texts = [(inp.d_text[slot], inp.win[slot][0], inp.d_off.p, inp.d_len.p) for inp in ins]
            if check:  # 2b. the batch's records, file by file, then the pairs' names
                t_c = time.perf_counter()
                for inp, text in zip(ins, texts):
                    refused = refused or _check_records(rt, classifier, ctx.s_main, inp.path, text, n, inp.cursor, done, busy)
                if paired:
                    refused = refused or _check_pairs(rt, classifier, ctx.s_main, (fastq1, fastq2), texts, n, done)
                busy["check_s"] += time.perf_counter() - t_c
                if refused is not None:
                    break
                if last:  # (raised behind this batch, the last both files have)
                    refused = checks.count_error(fastq1, fastq2, done + n, ns[0] > ns[1])
            if n == 0:
                break
            done += n
            for inp, (k, nx) in zip(ins, found):  # 3. the cursors move behind the batch (the index counts from the window's start)
                if k:
                    inp.avg_record = nx / k
                inp.cursor += nx
                inp.release()  # uploaded: the host pages of this batch can go
            if not last:  # 4. the next batch's windows go up beside this batch's kernels
                fut = up.submit(upload_all, slot ^ 1)
            hs, blocks = ctx.batch(texts, n, t0)  # 5. pack -> classify -> gathers (-> deflate) -> the download starts
            if hs is None:
                break
            q_w.put((hs, blocks))  # 6. the writer waits for the copy and appends the blocks
            if last:
                break
            slot ^= 1
    except BaseException as e:  # noqa: BLE001
        errors.append(e)
    finally:
        if fut is not None:  # (the upload thread may still write a device window)
            try:
                fut.result()
            except BaseException:  # noqa: BLE001
                pass
        up.shutdown(wait=True)
        if writer is not None:
            q_w.put(None)
            writer.join()
        ctx.close()
        for inp in ins:
            inp.close()
    if timings is not None:
        busy["wall_s"] = time.perf_counter() - t_wall
        busy["threads"] = T
        timings.update(busy)
    if errors:
        raise errors[0]
    if refused is not None:
        raise refused


# ---- the device pipeline dealt over several contexts by byte spans (_io="device-deal") ----------------------------------
SPAN_MIN = 16
_SPAN_TAIL = 1 << 16  # the first tail behind a span; doubled while a record that starts in the span ends behind it
_AVG_RECORD = 330     # _Input.avg_record's start value
_DealRun = namedtuple("_DealRun", "rt L f layout S dev_gz gzip_level chain path check")  # what the workers and the writer of a run share


def default_span_bytes(batch_reads: int) -> int:
    """the span of a run that names none: what ``batch_reads`` records of 330 bytes take, rounded up to 64 KiB.  It never
    depends on the number of contexts: an input and a span size give the same spans, whatever they are dealt over."""
    return -(-(max(1, int(batch_reads)) * _AVG_RECORD) // 65536) * 65536


def span_bytes(v) -> int:
    """_span_bytes as execute_demultiplexing takes it: an int of at least 16 (ValueError otherwise)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < SPAN_MIN:
        raise ValueError(f"_span_bytes must be an int of at least {SPAN_MIN} bytes, got {v!r}")
    return int(v)


class _ChainFailed(Exception):
    """raised in a thread that waits on a _SpanChain another thread has failed (never the run's first error)"""


class _SpanChain:
    """What the threads of demux_device_dealt share, and nothing of HIP: the span counter, the phase chain and the
    reorder step in front of the writer.

    Span k is the input's bytes [kS, (k + 1)S).  Its phase is (newlines in front of it) mod 4: phase(0) = 0,
    phase(k + 1) = phase(k) + count(k).  A worker take()s a span, publish()es its newline count as soon as it has it,
    wait_phase()s for its own phase and hand_over()s the span's blocks (None for a span without a record start); the
    writer takes them with next_in_order(), in span order.  end_at(k): span k starts at or behind the input's end.

    No deadlock.  A worker blocks in two places only: in wait_phase, and on one of its own download slots (which the
    writer hands back once the span that holds it is written).  It publishes its span's count BEFORE either.  Let m be
    the lowest span that is not written.  Spans are taken in ascending order, so if nobody holds m nobody holds a
    later span either and every worker is free to take it.  Otherwise its worker waits for nothing later than m:
    phase(m) needs the counts of the spans below m, which are written and therefore published; the slots of that
    worker are held by spans it took before m, which are written, so the writer has handed them back.  Span m reaches
    the writer, and m grows.  Workers with later spans may wait on count(m), which m's worker publishes before it can
    block.  The reorder map holds at most the spans that hold a slot (two a context) and the empty ones between them.

    fail(exc) records the first error and wakes every waiter: take and wait_phase raise _ChainFailed, next_in_order
    returns None."""

    def __init__(self):
        self.cv = threading.Condition()
        self.errors: list = []
        self._next = 0
        self._end = None      # the input's spans, once a worker has met its end
        self._phase = [0]     # _phase[k], as far as the published counts chain
        self._counts = {}     # counts published ahead of a lower span's
        self._done = {}       # handed over, not yet the writer's turn
        self._written = 0

    def take(self):
        """-> the next span's number; None when the input is known to end in front of it"""
        with self.cv:
            if self.errors:
                raise _ChainFailed()
            if self._end is not None and self._next >= self._end:
                return None
            self._next += 1
            return self._next - 1

    def end_at(self, k: int) -> None:
        with self.cv:
            self._end = k if self._end is None else min(self._end, k)
            self.cv.notify_all()

    def publish(self, k: int, count: int) -> None:
        with self.cv:
            self._counts[k] = int(count)
            while len(self._phase) - 1 in self._counts:
                j = len(self._phase) - 1
                self._phase.append((self._phase[j] + self._counts.pop(j)) % 4)
            self.cv.notify_all()

    def wait_phase(self, k: int) -> int:
        with self.cv:
            while len(self._phase) <= k and not self.errors:
                self.cv.wait()
            if self.errors:
                raise _ChainFailed()
            return self._phase[k]

    def hand_over(self, k: int, item) -> None:
        with self.cv:
            self._done[k] = item
            self.cv.notify_all()

    def next_in_order(self):
        """-> (k, item) of the lowest span not yet written; None when every span is through, or after fail()"""
        with self.cv:
            while True:
                if self.errors:
                    return None
                if self._written in self._done:
                    self._written += 1
                    return self._written - 1, self._done.pop(self._written - 1)
                if self._end is not None and self._written >= self._end:
                    return None
                self.cv.wait()

    def ended(self) -> bool:
        """a worker has met the input's end"""
        with self.cv:
            return self._end is not None

    def fail(self, exc: BaseException) -> None:
        with self.cv:
            if not isinstance(exc, _ChainFailed) or not self.errors:
                self.errors.append(exc)
            self.cv.notify_all()


class _DealWorker:
    """One context of demux_device_dealt: a _Context (streams, result buffers, two pinned download slots), the span's text
    and line tables, and the thread that takes spans from ``run.chain`` until the input ends (``run``: what the call shares)."""

    def __init__(self, k: int, run: _DealRun, classifier):
        self.run, self.cl, self.rt = run, classifier, run.rt
        self.busy = {"upload_s": 0.0, "device_s": 0.0, "phase_wait_s": 0.0, "batches": 0}
        if run.check:
            self.busy.update(check_s=0.0, checked_records=0)
        self.ctx = _Context(run.rt, classifier, self.busy, run.layout, run.dev_gz, run.gzip_level, run.chain.errors)
        self.text, self.off, self.len = _DevBuf(run.rt), _DevBuf(run.rt), _DevBuf(run.rt)
        self.spans = self.max_reads = 0
        self.thread = threading.Thread(target=self.loop, name=f"bdx-deal-{k}")

    def tables(self, max_reads: int):
        self.max_reads = max_reads
        self.off.ensure(4 * max_reads * 8)
        self.len.ensure(4 * max_reads * 4)

    def upload(self, start: int, want: int):
        """bytes [start, start + want) of the input (what is there of them) -> (bytes, final); None behind its end"""
        t0 = time.perf_counter()
        got = _upload_text(self.rt, self.run.L, self.run.f, self.ctx.s_copy, self.text, start, want, or_none=True)
        if got is not None:
            self.busy["upload_s"] += time.perf_counter() - t0
        return got

    def span(self, k: int) -> bool:
        """span k through this context -> False when the input ends in front of it"""
        run, chain, cl, lib = self.run, self.run.chain, self.cl, self.cl.lib
        S = run.S
        start, tail = k * S, _SPAN_TAIL
        up = self.upload(start, S + tail)
        if up is None:
            chain.end_at(k)
            return False
        self.spans += 1
        nbytes, final = up
        span_len = min(S, nbytes)
        starts_line = 1 if start == 0 else int(C.c_ubyte.from_address(run.L.bdx_fq_data(run.f.h) + start - 1).value == 10)
        t0 = time.perf_counter()
        d_text = self.text.p
        count = C.c_int64(0)
        cl._check(lib.bdx_fq_count_lines_device(cl.h, d_text, span_len, C.byref(count)))
        chain.publish(k, count.value)  # at once: the spans behind this one wait for nothing else of it
        t1 = time.perf_counter()
        phase = chain.wait_phase(k)
        t2 = time.perf_counter()
        self.busy["phase_wait_s"] += t2 - t1
        waited = t2 - t1
        n, complete = C.c_int64(0), C.c_int32(1)
        while True:
            rc = lib.bdx_fq_index_span_device(cl.h, d_text, nbytes, span_len, phase, starts_line, int(final), self.max_reads,
                                              self.off.p, self.len.p, C.byref(n), C.byref(complete))
            if rc == _E_SPACE:  # more records than the tables hold: the call has said how many
                self.tables(int(n.value) + (int(n.value) >> 3))
                continue
            cl._check(rc)
            if complete.value:
                break
            tail *= 2  # a record that starts in the span ends behind the window: a longer tail
            t_up = time.perf_counter()
            nbytes, final = self.upload(start, S + tail)
            waited += time.perf_counter() - t_up
            d_text = self.text.p
        n = int(n.value)
        if n == 0:  # a line longer than the span, or no line of it begins a record: the writer passes it
            self.busy["device_s"] += time.perf_counter() - t0 - waited
            chain.hand_over(k, None)
            return True
        if run.check:  # the span's records; a failure goes to the writer in the span's place, which raises it in span order
            t_c = time.perf_counter()
            refused = _check_records(self.rt, cl, self.ctx.s_main, run.path, (d_text, nbytes, self.off.p, self.len.p), n, start, None,
                                     self.busy)
            self.busy["check_s"] += time.perf_counter() - t_c
            if refused is not None:
                self.busy["device_s"] += time.perf_counter() - t0 - waited
                chain.hand_over(k, refused)
                return True
        self.ctx.size_results(n)
        hs, blocks = self.ctx.batch([(d_text, nbytes, self.off.p, self.len.p)], n, t0 + waited)
        if hs is None:
            raise _ChainFailed()
        chain.hand_over(k, (self.ctx.slots, hs, blocks))
        return True

    def loop(self):
        chain = self.run.chain
        try:
            self.rt.check(self.rt.hipSetDevice(int(getattr(self.cl, "device", 0))), "hipSetDevice")
            self.tables(self.run.S // 128 + 64)
            while True:
                k = chain.take()
                if k is None or not self.span(k):
                    break
        except BaseException as e:  # noqa: BLE001 - the first one reaches the caller
            chain.fail(e)

    def close(self):
        self.ctx.close()  # (chooses the device for the frees below as well)
        for b in (self.text, self.off, self.len):
            b.free()


def _write_dealt(run: _DealRun, T: int, busy: dict):
    """The writer thread: the spans in span order, each one's blocks from its context's slot (_write_blocks hands it back)"""
    chain = run.chain
    try:
        for k, item in iter(chain.next_in_order, None):
            busy["spans"] += 1
            # every span up to k is uploaded; the span behind k still reads the byte in front of it
            run.f.release(max(0, (k + 1) * run.S - 1))
            if isinstance(item, BaseException):  # (_check) the span was refused: every span in front of it is written
                raise item
            if item is not None:
                _write_blocks(run.rt, run.L, run.layout, run.dev_gz, T, busy, *item)
    except BaseException as e:  # noqa: BLE001
        chain.fail(e)


def demux_device_dealt(fastq1: str, config, output_directory: str, prefix1: str, classifiers: list, batch_reads: int,
                       timings: Optional[dict] = None, gzip_device: bool = False, gzip_level: int = 1,
                       span_bytes: Optional[int] = None, check: bool = False) -> None:
    """The device pipeline of demux_device for ONE single-end input (plain, or a .gz the host inflates), dealt over the
    contexts ``classifiers`` by byte spans.  The text is cut into spans of ``span_bytes`` bytes (default:
    default_span_bytes(batch_reads)); a record belongs to the span its first line starts in (bdx_fq_index_span_device
    has the rule).  One worker thread per context takes the next span, uploads it with a tail, counts its newlines
    (bdx_fq_count_lines_device) and publishes the count, waits for its phase, then indexes, packs, classifies, gathers,
    deflates with ``gzip_device`` and gzip output, and starts the download; one writer thread appends the blocks in
    span order (_SpanChain).  Files, counters and reports are those of demux_device; the gzip members of
    ``gzip_device`` depend on the input and the span size alone, not on the contexts.  Device memory of a context:
    the span with its tail three times (text, packed reads, blocks; the members as well with ``gzip_device``), 48 bytes
    a record of line table and 16 of results, and the context's own scratch.
    ``check`` (_check): every span's records are held to the record rules after its index (bdx_fq_check_device); a span
    that fails hands its BdxError to the writer instead of blocks, which raises it when the spans in front of it are
    written.  The message names the record's byte offset in the text and no record number: the span chain carries
    phases, not record counts.  timings then also holds check_s and checked_records."""
    if not classifiers or not all(hasattr(c, "classify_device") for c in classifiers):
        raise ValueError("the device FASTQ pipeline (_io='device-deal') needs the HIP classifier")
    t_wall = time.perf_counter()
    L = _io()
    rt = _Runtime(classifiers[0].lib)
    T = nativeio._threads()
    S = int(span_bytes) if span_bytes is not None else default_span_bytes(batch_reads)
    layout = OutputLayout(config, output_directory, prefix1, "", False)
    dev_gz = bool(gzip_device) and bool(layout.gz)
    wbusy = {"download_s": 0.0, "write_s": 0.0, "spans": 0}
    f = nativeio.FastqFile(fastq1)
    run = _DealRun(rt, L, f, layout, S, dev_gz, int(gzip_level), _SpanChain(), fastq1, bool(check))
    chain = run.chain
    workers = [_DealWorker(k, run, c) for k, c in enumerate(classifiers)]
    started = []
    writer = None
    try:
        for w in workers:
            w.ctx.open()
        writer = threading.Thread(target=_write_dealt, name="bdx-deal-writer", args=(run, T, wbusy))
        writer.start()
        for w in workers:
            w.thread.start()
            started.append(w)
        for w in started:
            w.thread.join()
        if not chain.errors and not chain.ended():  # (every worker left without meeting the end: cannot happen)
            chain.fail(BdxError("the span workers ended in front of the input's end"))
    except BaseException as e:  # noqa: BLE001
        chain.fail(e)
    finally:
        for w in started:
            w.thread.join()
        if writer is not None:
            if not started:
                chain.end_at(0)
            writer.join()
        for w in workers:
            try:
                w.close()
            except BaseException as e:  # noqa: BLE001
                chain.fail(e)
        f.close()
    if timings is not None:
        busy = dict(wbusy)
        for w in workers:
            for name, v in w.busy.items():
                busy[name] = v if name == "gzip_level" else busy.get(name, 0) + v
        busy["spans_per_device"] = [w.spans for w in workers]
        busy["span_bytes"] = S
        busy["wall_s"] = time.perf_counter() - t_wall
        busy["threads"] = T
        timings.update(busy)
    if chain.errors:
        raise chain.errors[0]
