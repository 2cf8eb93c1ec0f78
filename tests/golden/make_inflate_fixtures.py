"""Writes tests/golden/inflate/*.gz: size-tagged gzip members whose DEFLATE bodies come from libdeflate, the library
bgzip / htslib are normally linked against (it run-length-codes the two alphabets' code lengths as one array, so runs
cross their boundary, and builds codes and splits blocks in its own way — none of which zlib's encoder does).  The bodies are data: the tests read
the files and never the library, which need not be there when they run.

    python tests/golden/make_inflate_fixtures.py        (needs libdeflate.so.0)

Levels 1, 6, 9 and 12 of a 20 000-byte FASTQ-like text, 300 random bytes, a period-4 text and a text of runs (period 1 to
4, 499 bytes each, 7 letters between two): the last gives length symbols 284 and 285 and the first distance symbols one
code length, which libdeflate writes as one run across the boundary of the two alphabets (at levels 1 and 9).  One
65 280-byte FASTQ-like member (BGZF's block size) at level 6; the empty member."""
import ctypes as C
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import inflate_cases as IC  # noqa: E402


def compressor():
    L = C.CDLL("libdeflate.so.0")
    L.libdeflate_alloc_compressor.restype = C.c_void_p
    L.libdeflate_alloc_compressor.argtypes = [C.c_int]
    L.libdeflate_deflate_compress.restype = C.c_size_t
    L.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.libdeflate_deflate_compress_bound.restype = C.c_size_t
    L.libdeflate_deflate_compress_bound.argtypes = [C.c_void_p, C.c_size_t]
    L.libdeflate_free_compressor.argtypes = [C.c_void_p]

    def compress(plain: bytes, level: int) -> bytes:
        c = L.libdeflate_alloc_compressor(level)
        assert c
        try:
            cap = L.libdeflate_deflate_compress_bound(c, len(plain))
            buf = C.create_string_buffer(cap)
            n = L.libdeflate_deflate_compress(c, plain, len(plain), buf, cap)
            assert n > 0
            return buf.raw[:n]
        finally:
            L.libdeflate_free_compressor(c)

    return compress


def runs_text(n=20000, run=499, noise=7):
    rng = np.random.default_rng(noise * 1000 + run)
    out, size, k = [], 0, 0
    while size < n:
        unit = (b"A", b"AC", b"ACG", b"ACGT")[k % 4]
        out.append((unit * run)[:run] + rng.choice(np.frombuffer(b"ACGTN#:FI\n", dtype=np.uint8), noise).tobytes())
        size += len(out[-1])
        k += 1
    return b"".join(out)[:n]


def main():
    compress = compressor()
    out = os.path.join(HERE, "inflate")
    os.makedirs(out, exist_ok=True)
    texts = {"fastq_20000": IC.fastq_text(20000, 101), "random_300": IC.random_bytes(300, 102), "period4_20000": b"ACGT" * 5000,
             "runs_20000": runs_text()}
    jobs = [("l%02d_%s" % (level, name), text, level) for level in (1, 6, 9, 12) for name, text in texts.items()]
    jobs += [("l06_fastq_65280", IC.fastq_text(65280, 103), 6), ("l06_empty", b"", 6)]
    for name, text, level in jobs:
        comp = IC.wrap(compress(text, level), IC.trailer(text))
        assert gzip.decompress(comp) == text and len(comp) < 1 << 20
        with open(os.path.join(out, name + ".gz"), "wb") as f:
            f.write(comp)
        print("%-22s %6d -> %6d bytes" % (name, len(text), len(comp)))


if __name__ == "__main__":
    main()
