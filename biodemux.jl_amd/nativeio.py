"""Native host-side FASTQ reader / packer / in-order demux writer (csrc/bdx_io.cpp, libbdx_io.so).

SURVEY.md §8(f) rank 1 — the callers either side of the hot path (reader_task / writer_task,
core.jl:43-110, :118-224).  Same observable behaviour as the pure-Python path in core.py (which
stays as the reference implementation the tests cross-check against); the hot path in between is
the same single C-ABI call per batch.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import subprocess
import threading
import time
from typing import Optional

import numpy as np

from . import checks
from .hipabi import BdxError
from .outputs import OutputLayout

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "bdx_io.cpp")
_DEPS = (_SRC, os.path.join(_HERE, "csrc", "bdx_pool.h"))
LIB_PATH = os.path.join(_HERE, "csrc", "libbdx_io.so")
_lib = None


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(LIB_PATH) < os.path.getmtime(d) for d in _DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", LIB_PATH, _SRC, "-lz"])
    return LIB_PATH


def available() -> bool:
    return os.path.exists(LIB_PATH)


def _load():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.bdx_io_last_error.restype = C.c_char_p
        L.bdx_fq_open.restype = C.c_int32
        L.bdx_fq_open.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.bdx_fq_open_mt.restype = C.c_int32
        L.bdx_fq_open_mt.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp)]
        L.bdx_fq_parallel_inflate.restype = C.c_int32
        L.bdx_fq_parallel_inflate.argtypes = [vp]
        L.bdx_fq_close.restype = None
        L.bdx_fq_close.argtypes = [vp]
        L.bdx_fq_size.restype = C.c_int64
        L.bdx_fq_size.argtypes = [vp]
        L.bdx_fq_index.restype = C.c_int64
        L.bdx_fq_index.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, C.POINTER(C.c_int64), C.c_int32]
        L.bdx_fq_release.restype = None
        L.bdx_fq_release.argtypes = [vp, C.c_int64]
        L.bdx_fq_seq_bytes.restype = C.c_int64
        L.bdx_fq_seq_bytes.argtypes = [vp, C.c_int64]
        L.bdx_fq_pack.restype = None
        L.bdx_fq_pack.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int32]
        L.bdx_fq_demux_write.restype = C.c_int32
        L.bdx_fq_demux_write.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int32, C.POINTER(C.c_char_p), vp, vp,
                                         C.c_int32, C.c_int32, C.c_int32]
        L.bdx_fq_demux_write_range.restype = C.c_int32
        L.bdx_fq_demux_write_range.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int32, C.POINTER(C.c_char_p), vp, vp,
                                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.bdx_fq_members_open.restype = C.c_int32
        L.bdx_fq_members_open.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
        L.bdx_fq_members_count.restype = C.c_int64
        L.bdx_fq_members_count.argtypes = [vp]
        L.bdx_fq_members_eligible.restype = C.c_int32
        L.bdx_fq_members_eligible.argtypes = [vp]
        L.bdx_fq_members_reason.restype = C.c_char_p
        L.bdx_fq_members_reason.argtypes = [vp]
        L.bdx_fq_members_data.restype = vp
        L.bdx_fq_members_data.argtypes = [vp]
        L.bdx_fq_members_size.restype = C.c_int64
        L.bdx_fq_members_size.argtypes = [vp]
        L.bdx_fq_members_table.restype = None
        L.bdx_fq_members_table.argtypes = [vp, vp, vp, vp]
        L.bdx_fq_members_release.restype = None
        L.bdx_fq_members_release.argtypes = [vp, C.c_int64]
        L.bdx_fq_members_close.restype = None
        L.bdx_fq_members_close.argtypes = [vp]
        L.bdx_fq_data.restype = vp
        L.bdx_fq_data.argtypes = [vp]
        L.bdx_fq_check.restype = C.c_int32
        L.bdx_fq_check.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32]
        L.bdx_fq_check_pair.restype = C.c_int32
        L.bdx_fq_check_pair.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]
        _lib = L
    return _lib


def _threads() -> int:
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = max(1, min(n, int(int(q) / int(p) + 0.5)))
    except Exception:
        pass
    return max(1, min(n, 32))


class FastqFile:
    def __init__(self, path: str, nthreads: int = 0):
        """``nthreads``: inflate threads for size-tagged .gz member chains (BGZF, this library's own output);
        0 = one per available core (at most 16).  Ordinary gzip streams are inflated by one thread."""
        self.L = _load()
        h = C.c_void_p()
        if self.L.bdx_fq_open_mt(path.encode(), int(nthreads), C.byref(h)) != 0:
            raise OSError(self.L.bdx_io_last_error().decode())
        self.h = h
        self.cursor = 0

    @property
    def size(self) -> int:
        """Total bytes (a .gz input is inflated in the background: this waits for the end of the stream)."""
        return int(self.L.bdx_fq_size(self.h))

    @property
    def parallel_inflate(self) -> bool:
        """True when the .gz input was a size-tagged member chain inflated block-parallel (waits for the end)."""
        return bool(self.L.bdx_fq_parallel_inflate(self.h))

    def release(self, upto: int) -> None:
        """Records below byte `upto` are written out: a streamed .gz input gives their pages back."""
        self.L.bdx_fq_release(self.h, int(upto))

    def next_batch(self, max_reads: int, nthreads: int, off=None, ln=None):
        """-> (n_records, line_off int64[4n], line_len int32[4n]) from the cursor on.  ``off`` / ``ln``: arrays to reuse
        (a fresh 48 MB pair per 2^20-read batch is page-faulted in by the indexer)."""
        if off is None or len(off) < 4 * max_reads:
            off = np.empty(4 * max_reads, dtype=np.int64)
        if ln is None or len(ln) < 4 * max_reads:
            ln = np.empty(4 * max_reads, dtype=np.int32)
        nxt = C.c_int64(0)
        n = int(self.L.bdx_fq_index(self.h, self.cursor, max_reads, off.ctypes.data, ln.ctypes.data, C.byref(nxt),
                                    nthreads))
        if n < 0:
            raise OSError(self.L.bdx_io_last_error().decode())
        self.cursor = int(nxt.value)
        return n, off, ln

    def pack(self, off, ln, n: int, nthreads: int, seq=None, so=None):
        total = int(self.L.bdx_fq_seq_bytes(ln.ctypes.data, n))
        if seq is None or len(seq) < max(total, 1):
            seq = np.empty(max(total, 1) + (max(total, 1) >> 4), dtype=np.uint8)
        if so is None or len(so) < n + 1:
            so = np.empty(n + 1, dtype=np.int64)
        self.L.bdx_fq_pack(self.h, off.ctypes.data, ln.ctypes.data, n, seq.ctypes.data, so.ctypes.data, nthreads)
        return (seq[:total] if total else np.zeros(0, dtype=np.uint8)), so[:n + 1]

    def check(self, off, ln, n: int, rules: int, nthreads: int):
        """bdx_fq_check over the first n records of a line table -> (first_bad, broken): the lowest record that breaks a
        rule of ``rules`` and the rules it breaks, or (-1, 0)"""
        bad, broken = C.c_int64(-1), C.c_int32(0)
        if self.L.bdx_fq_check(self.h, off.ctypes.data, ln.ctypes.data, n, rules, C.byref(bad), C.byref(broken), nthreads) != 0:
            raise BdxError(self.L.bdx_io_last_error().decode())
        return int(bad.value), int(broken.value)

    def check_pair(self, off, ln, other: "FastqFile", off2, ln2, n: int, nthreads: int) -> int:
        """bdx_fq_check_pair -> the lowest record whose read name differs from the same record's of ``other``, or -1"""
        bad = C.c_int64(-1)
        if self.L.bdx_fq_check_pair(self.h, off.ctypes.data, ln.ctypes.data, other.h, off2.ctypes.data, ln2.ctypes.data, n,
                                    C.byref(bad), nthreads) != 0:
            raise BdxError(self.L.bdx_io_last_error().decode())
        return int(bad.value)

    def line(self, off, ln, k: int) -> bytes:
        """line k of a line table, from the host text"""
        return C.string_at(self.L.bdx_fq_data(self.h) + int(off[k]), int(ln[k]))

    def close(self):
        if self.h:
            self.L.bdx_fq_close(self.h)
            self.h = None


class GzMembers:
    """A .gz file opened WITHOUT inflating it: its compressed bytes mapped (``data``, ``size``) and the member table of
    its size-tagged chain (BGZF 'B','C' or this library's 'D','X'): ``comp_off`` int64, ``comp_len`` and ``isize`` int32,
    one entry per member, and ``plain_off`` (n + 1 entries: the prefix sums of ISIZE, a member's place in the text).
    ``eligible``: every member is tagged, every ISIZE is at most ``member_max`` and the tags land on the file's end;
    otherwise ``reason`` says which member breaks which rule and the table holds the members before it."""

    def __init__(self, path: str, member_max: int):
        self.L = _load()
        h = C.c_void_p()
        if self.L.bdx_fq_members_open(path.encode(), int(member_max), C.byref(h)) != 0:
            raise OSError(self.L.bdx_io_last_error().decode())
        self.h = h
        self.path = path
        n = int(self.L.bdx_fq_members_count(h))
        self.comp_off = np.zeros(n, dtype=np.int64)
        self.comp_len = np.zeros(n, dtype=np.int32)
        self.isize = np.zeros(n, dtype=np.int32)
        self.L.bdx_fq_members_table(h, self.comp_off.ctypes.data, self.comp_len.ctypes.data, self.isize.ctypes.data)
        self.plain_off = np.concatenate([[0], np.cumsum(self.isize, dtype=np.int64)]).astype(np.int64)
        self.eligible = bool(self.L.bdx_fq_members_eligible(h))
        self.reason = self.L.bdx_fq_members_reason(h).decode()
        self.data = int(self.L.bdx_fq_members_data(h) or 0)
        self.size = int(self.L.bdx_fq_members_size(h))

    def __len__(self) -> int:
        return len(self.comp_off)

    def release(self, upto: int) -> None:
        """The compressed bytes below `upto` are uploaded: their pages can go."""
        self.L.bdx_fq_members_release(self.h, int(upto))

    def close(self):
        if self.h:
            self.L.bdx_fq_members_close(self.h)
            self.h = None


# Batch buffers of finished runs (line tables, the packed chunk, verdict vectors: ~120 MB per set at 2^19 reads of 150 bases,
# five sets in flight).  A run takes its sets from here and puts them back: the next execute_demultiplexing of the process
# neither allocates nor page-faults them again, and a run's return does not spend 30 ms giving 600 MB back to the kernel
# (measured: 10 M reads, 0.326 s per call of which 0.030 s after the last batch was written).  `release_buffers()` empties it.
# A run over several device contexts takes more sets (see demux_native) but gives back at most _BUFFER_POOL_MAX: the pool
# keeps what one single-device run needs, not N times that.  Concurrent runs of one process share it under _BUFFER_POOL_LOCK.
_BUFFER_POOL: list = []
_BUFFER_POOL_MAX = 5
_BUFFER_POOL_LOCK = threading.Lock()


def release_buffers() -> None:
    """Drop the batch buffers kept from finished runs (a long-running host that is done demultiplexing)."""
    with _BUFFER_POOL_LOCK:
        del _BUFFER_POOL[:]


class _Batch:
    """One batch on its way reader -> classify -> writer: its id (the input order), ``n`` records, the line tables of both
    inputs, the packed chunk (``seq``, ``so``), the inputs' cursors behind it, the buffer set ``buf`` all these arrays
    belong to and — once classified — the output class of every read (``cls``), what is kept of it (``ks``, ``ke``) and the
    classes in use (``used``)."""
    __slots__ = ("bid", "n", "off1", "ln1", "off2", "ln2", "seq", "so", "cur1", "cur2", "buf", "cls", "ks", "ke", "used")

    def __init__(self, bid, n, off1, ln1, off2, ln2, seq, so, cur1, cur2, buf):
        self.bid, self.n, self.off1, self.ln1, self.off2, self.ln2 = bid, n, off1, ln1, off2, ln2
        self.seq, self.so, self.cur1, self.cur2, self.buf = seq, so, cur1, cur2, buf
        self.cls = self.ks = self.ke = self.used = None


class _NativeRun:
    """The threads of one demux_native call and what they share: reader -> q_in -> one classify thread per context -> the
    reorder step -> q_out -> writer, and the batch buffer sets coming back through ``free``."""

    def __init__(self, fastq1, fastq2, layout, classifiers, batch_reads, on_batch, check=False):
        self.layout, self.classifiers, self.batch_reads, self.on_batch = layout, classifiers, batch_reads, on_batch
        N = len(classifiers)
        self.busy = {"index_s": 0.0, "pack_s": 0.0, "classify_s": 0.0, "write_s": 0.0, "batches": 0}
        self.paths, self.check = (fastq1, fastq2), bool(check)
        # a failed check (_check): raised once every batch in front of it is written — it is no entry of ``errors``, at the
        # sight of which the classify threads drop what they hold
        self.refused: Optional[BaseException] = None
        if check:
            self.busy.update(check_s=0.0, checked_records=0)
        self.L = _load()
        self.T = _threads()
        # (developer knobs: host threads of the reader's / the writer's parallel sections — both default to the whole quota)
        self.TR = max(1, int(os.environ.get("BDX_IO_READER_THREADS", self.T)))
        self.TW = max(1, int(os.environ.get("BDX_IO_WRITER_THREADS", self.T)))
        self.f1 = FastqFile(fastq1)
        self.f2 = FastqFile(fastq2) if fastq2 is not None else None
        self.errors: list = []
        self.q_in: "queue.Queue" = queue.Queue(maxsize=1)
        # (the reorder step puts into this under its lock: it must never block — the batch sets bound it)
        self.q_out: "queue.Queue" = queue.Queue()
        self.per_dev_s = [0.0] * N
        self.per_dev_b = [0] * N
        self.parked: dict = {}  # batch id -> batch, for results that finished before an older batch
        self.next_id = 0
        self.order_lock = threading.Lock()
        self.batch_lock = threading.Lock()  # serialises on_batch (the summary of an injected classifier)
        # Batch buffers travel reader -> classify -> writer and come back through `free`: line tables, the packed chunk and
        # the verdict vectors are allocated a handful of times per run, not once per batch (fresh arrays of this size are
        # page-faulted in by whoever writes them first: ~15 % of the reader's time)
        self.free: "queue.Queue" = queue.Queue()
        # N contexts: 1 being filled by the reader + 1 waiting in q_in + N in the contexts + N - 1 results parked early in the
        # reorder step (while the oldest batch is still being classified) + 1 being written + 1 queued for the writer = 2N + 3.
        # (One context: 5 — one set per stage (reader, classify, writer) + one waiting in front of each of the two consumers.)
        # The count only decides how much overlaps; the dealer cannot deadlock with any count >= 1: every set is owned by a
        # batch that was read and is not yet written.  If the reader waits for a set, let r be the oldest of those batches.
        # Every batch before r is written, so r is never parked: it is in q_in or in a context (which classify it without
        # waiting for anything: the reorder step and the writer's queue are unbounded, their size is bounded by the sets),
        # or with the writer.  Either way r reaches the disk and its set comes back.
        n_sets = 2 * N + 3
        with _BUFFER_POOL_LOCK:
            self.bufs = [(_BUFFER_POOL.pop() if _BUFFER_POOL else {}) for _ in range(n_sets)]
        for b in self.bufs:
            self.free.put(b)

    def give_back(self, batch: _Batch) -> None:
        """A batch that will not be written (an error somewhere): its buffer set goes back to the reader."""
        self.free.put(batch.buf)

    def reader(self):
        f1, f2, TR, busy = self.f1, self.f2, self.TR, self.busy
        uneven = None  # (_check) the files of a pair hold different numbers of records: raised behind the last common batch
        try:
            bid = done = 0
            while True:
                # (a batch dropped on an error path never comes back through `free`: poll, and stop once anything failed —
                # the reader must always reach its final q_in.put(None), or the classify threads wait for it forever)
                while True:
                    try:
                        buf = self.free.get(timeout=0.05)
                        break
                    except queue.Empty:
                        if self.errors:
                            return
                if self.errors:
                    return
                t0 = time.perf_counter()
                n1, off1, ln1 = f1.next_batch(self.batch_reads, TR, buf.get("off1"), buf.get("ln1"))
                buf["off1"], buf["ln1"] = off1, ln1
                off2 = ln2 = None
                if f2 is not None:
                    n2, off2, ln2 = f2.next_batch(self.batch_reads, TR, buf.get("off2"), buf.get("ln2"))
                    buf["off2"], buf["ln2"] = off2, ln2
                    n = min(n1, n2)  # lock-step pairs: stop at the shorter file (core.jl:48)
                    last = n1 != n2
                else:
                    n, last = n1, False
                if self.check:
                    tc = time.perf_counter()
                    self.refused = self.check_batch(done, n, off1, ln1, off2, ln2)
                    if self.refused is None and f2 is not None and n1 != n2:
                        uneven = checks.count_error(*self.paths, done + n, n1 > n2)
                    busy["check_s"] += time.perf_counter() - tc
                    if self.refused is not None:
                        break
                    t0 += time.perf_counter() - tc  # (index_s does not count it)
                if n == 0:
                    break
                done += n
                t1 = time.perf_counter()
                seq, so = f1.pack(off1, ln1, n, TR, buf.get("seq"), buf.get("so"))
                if seq.base is not None:
                    buf["seq"] = seq.base
                if so.base is not None:
                    buf["so"] = so.base
                busy["index_s"] += t1 - t0
                busy["pack_s"] += time.perf_counter() - t1
                self.q_in.put(_Batch(bid, n, off1, ln1, off2, ln2, seq, so, f1.cursor, f2.cursor if f2 is not None else 0, buf))
                bid += 1
                if last:
                    break
            if self.refused is None:
                self.refused = uneven
        except BaseException as e:  # noqa: BLE001 - forwarded to the caller
            self.errors.append(e)
        finally:
            self.q_in.put(None)

    def check_batch(self, done: int, n: int, off1, ln1, off2, ln2):
        """_check: the first n records of the batch (``done`` records lie in front of it) against the record rules, file 1
        then file 2, then the pairs' names (bdx_fq_check, bdx_fq_check_pair) -> the BdxError of the first failure, or None"""
        files = ((self.paths[0], self.f1, off1, ln1),) + (((self.paths[1], self.f2, off2, ln2),) if self.f2 is not None else ())
        for path, f, off, ln in files:
            bad, broken = f.check(off, ln, n, checks.ALL_RULES, self.TR)
            self.busy["checked_records"] += n
            if bad >= 0:
                return checks.record_error(path, done + bad + 1, int(off[4 * bad]), broken, int(ln[4 * bad + 1]), int(ln[4 * bad + 3]))
        if self.f2 is not None:
            bad = self.f1.check_pair(off1, ln1, self.f2, off2, ln2, n, self.TR)
            if bad >= 0:
                return checks.pair_error(*self.paths, done + bad + 1, self.f1.line(off1, ln1, 4 * bad), self.f2.line(off2, ln2, 4 * bad))
        return None

    def classify(self, cl, b: _Batch):
        """One batch through one context: fills in the batch's classes -> (verdicts, seconds in classify)."""
        buf, n = b.buf, b.n
        tc0 = time.perf_counter()
        res = buf.get("out")
        reuse = (res is not None and len(res["bc1"]) >= n and getattr(cl, "want_pass", False) is False
                 and hasattr(cl, "lib"))  # (the HIP wrapper takes result arrays to reuse; test doubles may not)
        if reuse:
            out = cl.classify(b.seq, b.so, out={k: v[:n] for k, v in res.items()})  # <- the hot path: one C-ABI call per batch
        else:
            out = cl.classify(b.seq, b.so)
            if set(out) == {"bc1", "bc2", "keep_start", "keep_end"}:
                buf["out"] = out
        dt = time.perf_counter() - tc0
        cls = buf.get("cls")
        if cls is None or len(cls) < n:
            cls = buf["cls"] = np.empty(max(n, self.batch_reads), dtype=np.int32)
        b.cls = self.layout.classes(out["bc1"], out["bc2"], cls[:n])
        b.ks = np.ascontiguousarray(out["keep_start"], dtype=np.int32)
        b.ke = np.ascontiguousarray(out["keep_end"], dtype=np.int32)
        b.used = np.flatnonzero(np.bincount(b.cls, minlength=self.layout.n_classes))
        return out, dt

    def worker(self, k):
        """The classify thread of context k: takes the batches from the reader as they come (first free context wins)
        and hands the results to the writer strictly by batch id."""
        cl = self.classifiers[k]
        for b in iter(self.q_in.get, None):
            if self.errors:
                self.give_back(b)
                continue
            try:
                out, dt = self.classify(cl, b)
                if self.on_batch is not None:
                    with self.batch_lock:
                        self.on_batch(out)
            except BaseException as e:  # noqa: BLE001 - forwarded to the caller
                self.errors.append(e)
                self.give_back(b)
                continue
            self.per_dev_s[k] += dt
            self.per_dev_b[k] += 1
            with self.order_lock:  # release strictly by batch id: per-file order = input order (core.jl:139-148)
                self.parked[b.bid] = b
                while self.next_id in self.parked:
                    self.q_out.put(self.parked.pop(self.next_id))
                    self.next_id += 1
        self.q_in.put(None)  # the end mark goes on to the next worker (at most one is ever in the queue)

    def writer(self):
        """Gathers every batch straight into the (mapped) output files with all its threads working on all files
        (csrc/bdx_io.cpp): one writer thread, every class.  (bdx_fq_demux_write_range could let several writer threads
        share a batch by class range, which pays on file systems without shared writable mappings; no caller does.)"""
        L, f1, f2, lay = self.L, self.f1, self.f2, self.layout
        try:
            for b in iter(self.q_out.get, None):
                tw0 = time.perf_counter()
                for i, prefix, trim in lay.streams:
                    f, off, ln = (f1, b.off1, b.ln1) if i == 0 else (f2, b.off2, b.ln2)
                    rc = L.bdx_fq_demux_write_range(f.h, off.ctypes.data, ln.ctypes.data, b.n, b.cls.ctypes.data,
                                                    lay.n_classes, lay.c_paths(prefix, b.used), b.ks.ctypes.data,
                                                    b.ke.ctypes.data, int(trim), lay.gz, self.TW, 0, lay.n_classes)
                    if rc != 0:
                        raise OSError(L.bdx_io_last_error().decode())
                self.busy["write_s"] += time.perf_counter() - tw0
                f1.release(b.cur1)  # this batch and everything before it is on disk
                if f2 is not None:
                    f2.release(b.cur2)
                self.free.put(b.buf)
        except BaseException as e:  # noqa: BLE001
            self.errors.append(e)
            for b in iter(self.q_out.get, None):  # keep draining so nobody blocks; the dropped batches' buffers go back
                self.give_back(b)

    def run(self):
        tr = threading.Thread(target=self.reader, name="bdx-reader")
        tw = threading.Thread(target=self.writer, name="bdx-writer-0")
        tks = [threading.Thread(target=self.worker, args=(k,), name=f"bdx-classify-{k}") for k in range(len(self.classifiers))]
        tr.start()
        tw.start()
        try:
            for tk in tks:
                tk.start()
            for tk in tks:
                tk.join()
        except BaseException as e:  # noqa: BLE001
            self.errors.append(e)
            for tk in tks:  # (the workers drain q_in once they see the error, the reader stops on it)
                if tk.ident is not None:
                    tk.join()
            for b in iter(self.q_in.get, None):  # (what is left: everything, or — behind the workers — the end mark they passed on)
                self.give_back(b)
        finally:
            for b in self.parked.values():  # (only after an error: results behind a batch that never came)
                self.give_back(b)
            self.parked.clear()
            self.q_out.put(None)
            tr.join()
            tw.join()
            self.f1.close()
            if self.f2 is not None:
                self.f2.close()
            with _BUFFER_POOL_LOCK:
                for b in self.bufs:  # (every thread has been joined: nobody holds a set any more)
                    if len(_BUFFER_POOL) < _BUFFER_POOL_MAX:
                        _BUFFER_POOL.append(b)


def demux_native(fastq1: str, fastq2: Optional[str], config, output_directory: str, prefix1: str, prefix2: str,
                 classifiers: list, batch_reads: int, on_batch=None, timings: Optional[dict] = None,
                 check: bool = False) -> None:
    """Native counterpart of core._demux: index -> pack -> ONE C-ABI classify call -> in-order write, as a pipeline of
    threads (reader | one classify thread per context | writer; the native calls release the GIL).  The classify
    threads take the batches from the reader as they come free and a reorder step hands the results to the writer
    strictly by batch id, so per-file order is input order exactly as with the reference's single writer task
    (core.jl:139-148) and the files are those of a single context.  ``on_batch`` is called under a lock.
    ``check`` (_check): the reader holds every batch to the record rules and a paired one to the pair rule right after its
    index (bdx_fq_check, bdx_fq_check_pair on the reader's threads); at the first failure it reads no further, the batches
    in front of it go through classify and the writer as usual, and the BdxError is raised then; timings also holds
    check_s and checked_records."""
    t_wall = time.perf_counter()
    layout = OutputLayout(config, output_directory, prefix1, prefix2, fastq2 is not None)
    run = _NativeRun(fastq1, fastq2, layout, list(classifiers), batch_reads, on_batch, check)
    run.run()
    if timings is not None:  # busy seconds of the three overlapped stages (reader = index + pack | classify | writer)
        busy = run.busy
        busy["classify_s"] = sum(run.per_dev_s)  # (summed over the contexts, which overlap each other)
        busy["batches"] = sum(run.per_dev_b)
        if len(run.classifiers) > 1:
            busy["classify_s_per_device"] = run.per_dev_s
            busy["batches_per_device"] = run.per_dev_b
        busy["wall_s"] = time.perf_counter() - t_wall
        busy["threads"] = run.T
        timings.update(busy)
    if run.errors:
        raise run.errors[0]
    if run.refused is not None:
        raise run.refused
