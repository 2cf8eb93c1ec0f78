"""The device FASTQ pipeline (_io="device") off the GPU: it refuses anything but the HIP classifier (no silent fallback
to the host pipeline), fails loudly without a device, and its host half — bdx_fq_write_blocks, bdx_fq_wait — writes
and waits like the native writer / reader."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import helpers as H
from biodemux_jl_amd import deviceio, nativeio


@pytest.fixture(scope="module", autouse=True)
def _built():
    nativeio.build()


def _small(tmp_path):
    fq = tmp_path / "reads.fastq"
    fq.write_text("@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nTTTTACGT\n+\nIIIIIIII\n")
    bc = tmp_path / "bc.fasta"
    bc.write_text(">BC1\nACGT\n")
    return str(fq), str(bc)


def test_device_io_refuses_an_injected_classifier(tmp_path):
    fq, bc = _small(tmp_path)
    with pytest.raises(ValueError, match="device FASTQ pipeline needs the HIP classifier"):
        H.bdx.execute_demultiplexing(fq, bc, str(tmp_path / "out"), _classifier_factory=H.oracle_factory, _io="device")
    assert not os.path.exists(tmp_path / "out" / "reads.BC1.fastq")


def test_device_io_without_gpu_raises_bdx_error(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    fq, bc = _small(tmp_path)
    with pytest.raises(H.bdx.BdxError):
        H.bdx.execute_demultiplexing(fq, bc, str(tmp_path / "out"), _io="device")


def _blocks(sizes, seed=1):
    rng = np.random.default_rng(seed)
    parts = [bytes(rng.integers(65, 91, size=s, dtype=np.uint8)) for s in sizes]
    return parts, np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8).copy(), np.asarray(sizes, dtype=np.int64)


@pytest.mark.parametrize("gz", [0, 1])
def test_write_blocks_appends_each_class_to_its_file(tmp_path, gz):
    L = deviceio._io()
    sizes = [3, 0, 11, (5 << 20) + 17, 0, 1]  # one class spans two 4 MiB gzip members
    paths = [str(tmp_path / (f"c{c}.fastq.gz" if gz else f"c{c}.fastq")) for c in range(len(sizes))]
    arr = (C.c_char_p * len(sizes))(*[p.encode() if s else None for p, s in zip(paths, sizes)])
    want = {}
    for batch in range(2):  # appended in batch order
        parts, buf, cb = _blocks(sizes, seed=batch)
        assert L.bdx_fq_write_blocks(buf.ctypes.data, cb.ctypes.data, len(sizes), arr, gz, 4) == 0
        for p, part in zip(paths, parts):
            want[p] = want.get(p, b"") + part
    for p, s in zip(paths, sizes):
        if not s:
            assert not os.path.exists(p), "a class without bytes creates no file"
            continue
        got = open(p, "rb").read()
        assert (gzip.decompress(got) if gz else got) == want[p]
    if gz:  # the members carry the 'D','X' size tag: this library's parallel inflate reads them back
        f = nativeio.FastqFile(paths[3], 4)
        try:
            assert f.parallel_inflate and f.size == len(want[paths[3]])
        finally:
            f.close()


def test_write_blocks_reports_failures(tmp_path):
    L = deviceio._io()
    _, buf, cb = _blocks([4, 4])
    arr = (C.c_char_p * 2)(str(tmp_path / "a").encode(), str(tmp_path / "missing_dir" / "b").encode())
    assert L.bdx_fq_write_blocks(buf.ctypes.data, cb.ctypes.data, 2, arr, 0, 2) != 0
    assert b"cannot write" in L.bdx_io_last_error()
    arr = (C.c_char_p * 2)(str(tmp_path / "a").encode(), None)
    assert L.bdx_fq_write_blocks(buf.ctypes.data, cb.ctypes.data, 2, arr, 0, 2) != 0


def test_wait_on_plain_and_streamed_input(tmp_path):
    L = deviceio._io()
    text = b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in range(20000))
    plain = tmp_path / "x.fastq"
    plain.write_bytes(text)
    gzp = tmp_path / "x.fastq.gz"
    gzp.write_bytes(gzip.compress(text))
    for p in (plain, gzp):
        f = nativeio.FastqFile(str(p))
        try:
            avail, fin = C.c_int64(), C.c_int32()
            assert L.bdx_fq_wait(f.h, 1 << 40, C.byref(avail), C.byref(fin)) == 0
            assert fin.value == 1 and avail.value == len(text)
            data = C.string_at(L.bdx_fq_data(f.h), avail.value)
            assert data == text
        finally:
            f.close()
    bad = tmp_path / "bad.fastq.gz"
    blob = gzip.compress(text)
    bad.write_bytes(blob[: len(blob) // 2] + b"\0" * 64 + blob[len(blob) // 2 + 64:])
    f = nativeio.FastqFile(str(bad))
    try:
        avail, fin = C.c_int64(), C.c_int32()
        assert L.bdx_fq_wait(f.h, 1 << 40, C.byref(avail), C.byref(fin)) == -1
    finally:
        f.close()
