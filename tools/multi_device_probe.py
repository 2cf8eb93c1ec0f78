#!/usr/bin/env python3
"""Dealer overhead of execute_demultiplexing(..., devices=[...]) on ONE GPU (GPU box): a classify-bound config through the
native pipeline with devices=[0] and devices=[0, 0], alternating, in one process.

  N=200000 REPS=2 python tools/multi_device_probe.py [out.json]

48 barcodes of 160 nt (longer than 128 nt: the unfiltered exact kernel), N synthetic reads of 250 nt, max_error_rate=0.1,
25 000-read batches, input and outputs on tmpfs (/dev/shm when present).  Every run prints its wall seconds, the peak
thread count of the process (sampled from /proc/self/status every 5 ms) and its _timings; both settings must give the same
counters.  Two contexts on one GPU show only what dealing costs or overlaps; a speedup needs distinct GPUs."""
import json
import os
import shutil
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    import biodemux_jl_amd as bdx
    from biodemux_jl_amd import synth

    n = int(os.environ.get("N", 200_000))
    reps = int(os.environ.get("REPS", 2))
    bcs = synth.make_barcodes(48, 160, seed=5)
    seq, off, _ = synth.make_reads(bcs, n, 250, seed=6)
    tmp = tempfile.mkdtemp(prefix="bdx_multi_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    peak = [0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            with open("/proc/self/status") as f:
                for line in f:
                    if line.startswith("Threads:"):
                        peak[0] = max(peak[0], int(line.split()[1]))
            time.sleep(0.005)

    sampler = threading.Thread(target=sample, daemon=True)
    runs = []
    try:
        fq = os.path.join(tmp, "reads.fastq")
        with open(fq, "wb") as f:
            f.write(b"".join(b"@r%d\n" % i + seq[off[i]:off[i + 1]].tobytes() + b"\n+\n" + b"F" * 250 + b"\n"
                             for i in range(n)))
        bc = os.path.join(tmp, "bc.csv")
        with open(bc, "w") as f:
            f.write("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
        sampler.start()
        for rep in range(reps):
            for devs in ([0], [0, 0]):
                out = os.path.join(tmp, f"out_{rep}_{len(devs)}")
                t = {}
                peak[0] = 0
                t0 = time.perf_counter()
                st = bdx.execute_demultiplexing(fq, bc, out, max_error_rate=0.1, devices=devs, _io="native",
                                                _batch_reads=25_000, _timings=t)
                r = dict(rep=rep, devices=devs, wall_s=round(time.perf_counter() - t0, 4), peak_threads=peak[0],
                         total_reads=st.total_reads, matched_reads=st.matched_reads,
                         timings={k: (round(v, 4) if isinstance(v, float) else
                                      [round(x, 4) for x in v] if isinstance(v, list) and v and isinstance(v[0], float)
                                      else v) for k, v in t.items()})
                print(json.dumps(r), flush=True)
                runs.append(r)
                shutil.rmtree(out)
    finally:
        stop.set()
        shutil.rmtree(tmp, ignore_errors=True)
    if len({(r["total_reads"], r["matched_reads"]) for r in runs}) != 1:
        print("counters differ between the settings", file=sys.stderr)
        return 1
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(n_reads=n, read_len=250, barcodes="48 x 160 nt", batch_reads=25_000, runs=runs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
