#!/usr/bin/env python3
"""Seed hits, resolve passes, append layers and sweep records per tile of the headline wave kernel on the C2 batch, counted on
the CPU from the seed pieces and bench.py's synthetic reads (no GPU).

    python tools/wave_hit_census.py [--reads 1000000] [--first-read 0]

Model of csrc/bdx_wave_kernel.h, headline form (32-read tiles of 150-base reads: 4800 flat positions, 300 groups of sixteen, one
scan round of five trips): a position is a hit when the eight 2-bit codes (byte >> 1) & 3 from it on are a piece of some barcode
(pieces of 8 at barcode offsets 0, 8, 16: build_wave_tables) — also where the eight bases straddle two reads (the scan queues
such a position, the resolve drops it).  The resolve takes 64 hits per pass; the append's serial loops run once per hit of the
fullest lane (lane = groups g, g + 64, ... of the tile); a record is a (read, barcode, cluster of diagonals within kb = 2 of its
first), the sweeps take 64 records per pass.  Positions whose eight bases run past the tile's end are left out (the image
behind the tile is padding)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from biodemux_jl_amd import synth  # noqa: E402

RW, LEN, Q, KB, M = 32, 150, 8, 2, 24


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--first-read", type=int, default=0)
    args = ap.parse_args()
    n = args.reads // RW * RW
    bcs = synth.make_barcodes(96, M, seed=synth.SEED)
    seq, off, _ = synth.make_reads(bcs, n, LEN, seed=synth.SEED, first_read=args.first_read)
    assert len(seq) == n * LEN
    w = (1 << (2 * np.arange(Q))).astype(np.uint32)
    # key -> (barcode, piece start) of the first piece with that key (two pieces with one key are rare; the census says how many)
    piece_of = {}
    dup = 0
    for b, bc in enumerate(bcs):
        code = (np.frombuffer(bc.encode(), dtype=np.uint8) >> 1) & 3
        for t in range(KB + 1):
            key = int((code[t * Q:t * Q + Q].astype(np.uint32) * w).sum())
            dup += key in piece_of
            piece_of.setdefault(key, (b, t * Q))
    present = np.zeros(1 << (2 * Q), dtype=bool)
    present[list(piece_of)] = True
    key_bc = np.zeros(1 << (2 * Q), dtype=np.int32)
    key_ps = np.zeros(1 << (2 * Q), dtype=np.int32)
    for k, (b, ps) in piece_of.items():
        key_bc[k], key_ps[k] = b, ps

    span = RW * LEN
    ntiles = n // RW
    hits_t = np.zeros(ntiles, dtype=np.int64)
    inread_t = np.zeros(ntiles, dtype=np.int64)
    layers_t = np.zeros(ntiles, dtype=np.int64)
    rec_t = np.zeros(ntiles, dtype=np.int64)
    chunk = 2048  # tiles at a time
    for t0 in range(0, ntiles, chunk):
        t1 = min(ntiles, t0 + chunk)
        code = ((seq[t0 * span:t1 * span] >> 1) & 3).astype(np.uint32).reshape(t1 - t0, span)
        keys = np.zeros((t1 - t0, span - Q + 1), dtype=np.uint32)
        for k in range(Q):
            keys += code[:, k:span - Q + 1 + k] << (2 * k)
        hit = present[keys]
        tile, pos = np.nonzero(hit)
        hits_t[t0:t1] = hit.sum(axis=1)
        # the fullest lane of the round: lane = group mod 64, group = position // 16
        lane_hits = np.zeros((t1 - t0, 64), dtype=np.int64)
        np.add.at(lane_hits, (tile, (pos // 16) % 64), 1)
        layers_t[t0:t1] = lane_hits.max(axis=1)
        read, p = pos // LEN, pos % LEN
        ok = p + Q <= LEN
        np.add.at(inread_t, t0 + tile[ok], 1)
        k = keys[tile[ok], pos[ok]]
        diag = p[ok] - key_ps[k]
        order = np.lexsort((diag, key_bc[k], read[ok], tile[ok]))
        tl, rd, bc, dg = tile[ok][order], read[ok][order], key_bc[k][order], diag[order]
        # records: within one (tile, read, barcode) a hit further than kb from the record's first diagonal opens a new one
        new = np.ones(len(tl), dtype=bool)
        same = (tl[1:] == tl[:-1]) & (rd[1:] == rd[:-1]) & (bc[1:] == bc[:-1])
        first = dg.copy()
        for i in range(1, len(tl)):  # (a few million hits at most)
            if same[i - 1] and dg[i] - first[i - 1] <= KB:
                new[i] = False
                first[i] = first[i - 1]
        np.add.at(rec_t, t0 + tl[new], 1)

    def line(name, v):
        print("%-34s mean %7.2f  median %5.0f  p1 %4.0f  p99 %4.0f  max %4.0f" % (name, v.mean(), np.median(v), np.percentile(v, 1), np.percentile(v, 99), v.max()))

    print("C2 batch, reads %d .. %d: %d tiles of %d reads; %d pieces, %d distinct keys (%d shared)" % (
        args.first_read, args.first_read + n - 1, ntiles, RW, 96 * (KB + 1), len(piece_of), dup))
    line("hits queued per tile", hits_t)
    line("  of them inside one read", inread_t)
    rp = (hits_t + 63) // 64
    line("resolve passes per tile", rp)
    for k in range(0, 5):
        print("  tiles with %d resolve pass%s: %6.2f %%" % (k, "" if k == 1 else "es", 100.0 * (rp == k).mean()))
    print("  fill of the last resolve pass: mean %.1f of 64 lanes" % (hits_t - 64 * (rp - 1)).clip(0).mean())
    line("append layers per tile (fullest lane)", layers_t)
    line("records (= sweeps) per tile", rec_t)
    sp = (rec_t + 63) // 64
    line("sweep passes per tile", sp)


if __name__ == "__main__":
    main()
