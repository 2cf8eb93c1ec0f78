"""The output layout of a run: which class a verdict belongs to, which file a class goes to and which streams a batch
writes.  core._demux, nativeio.demux_native and deviceio.demux_device all ask this one place; the device gather kernel
(csrc/bdx_fastq.hip) gets ``stride`` and ``n_classes`` from here and does the same arithmetic on the GPU."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .classification import filename_for


class OutputLayout:
    """Class of a read: 0 unknown (bc1 == 0), 1 ambiguous (bc1 < 0), 2 + (bc1 - 1) * stride + (bc2 - 1) matched; a
    single-barcode run has stride 1 and bc2 == 0."""

    def __init__(self, config, output_directory: str, prefix1: str, prefix2: str, paired: bool):
        self.config = config
        self.output_directory = output_directory
        self.stride = max(1, len(config.bc_seqs2)) if config.is_dual else 1
        self.n_classes = 2 + len(config.bc_seqs) * self.stride
        self.gz = int(bool(config.gzip_output))
        do_trim = config.trim_side is not None or config.trim_side2 is not None  # core.jl:240
        # output streams of a batch: (input index, prefix, trim) — only R1 is ever trimmed
        if paired and config.classify_both:  # core.jl:175-185
            self.streams = [(0, prefix1, do_trim), (1, prefix2, False)]
        elif paired:  # core.jl:186-190
            self.streams = [(1, prefix2, False)]
        else:  # core.jl:191-196
            self.streams = [(0, prefix1, do_trim)]

    def classes(self, bc1, bc2, out):
        """The class of every read of a batch, written into ``out`` (int32, as long as ``bc1``)."""
        np.subtract(bc1, 1, out=out)
        if self.stride != 1:
            np.multiply(out, self.stride, out=out)
            out += np.maximum(bc2, 1)
            out += 1
        else:
            out += 2
        out[bc1 == 0] = 0
        out[bc1 < 0] = 1
        return out

    def verdict(self, c: int):
        """Class -> the (bc1, bc2) that filename_for takes."""
        if c == 0:
            return 0, 0
        if c == 1:
            return -1, 0
        b1, b2 = divmod(c - 2, self.stride)
        return b1 + 1, (b2 + 1 if self.config.is_dual else 0)

    def c_paths(self, prefix: str, used_classes):
        """The output file of every class in use, for the native writers: a ``char *[n_classes]``, NULL elsewhere."""
        arr = (C.c_char_p * self.n_classes)()
        for c in used_classes:
            name = prefix + "." + filename_for(self.config, *self.verdict(int(c)))
            arr[int(c)] = os.path.join(self.output_directory, name).encode()
        return arr
