#!/usr/bin/env python3
"""End-to-end reads/s of execute_demultiplexing on the C2 shape: the native host pipeline (_io="native") against the device
FASTQ pipeline (_io="device"), each run in a fresh child process (GPU box).

  N=10000000 REPS=3 python tools/e2e_device_probe.py [out.json]

One synthetic FASTQ of N 150 bp reads x 96 barcodes (24 bp), max_error_rate=0.1, on tmpfs (/dev/shm unless E2E_ROOT is
set); the outputs are checked (total bytes = input bytes).  Prints every run with its stage seconds, then the medians; the
optional argument receives the same as JSON."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(root: str, n: int) -> None:
    import numpy as np

    from biodemux_jl_amd import synth

    fq = os.path.join(root, "synthetic.fastq")
    if os.path.exists(fq) and os.path.getsize(fq) == n * 319:
        return
    bcs = synth.make_barcodes(96, 24, seed=synth.SEED)
    seq, _, _ = synth.make_reads(bcs, n, 150, seed=synth.SEED)
    rec = np.empty((n, 319), dtype=np.uint8)
    rec[:, 0:5] = np.frombuffer(b"@read", dtype=np.uint8)
    ids = np.arange(n, dtype=np.int64)
    for k in range(9):
        rec[:, 13 - k] = (ids // 10 ** k % 10 + 48).astype(np.uint8)
    rec[:, 14] = 10
    rec[:, 15:165] = seq.reshape(n, 150)
    rec[:, 165:168] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 168:318] = ord("F")
    rec[:, 318] = 10
    rec.tofile(fq)
    with open(os.path.join(root, "barcodes.csv"), "w") as f:
        f.write("ID,Full_seq,Full_annotation\n" + "".join(f"bc{i + 1:03d},{b},{'B' * 24}\n" for i, b in enumerate(bcs)))


def child(mode: str) -> None:
    import biodemux_jl_amd as bdx

    root = os.environ["E2E_ROOT"]
    n = int(os.environ["N"])
    fq, bc, out = (os.path.join(root, x) for x in ("synthetic.fastq", "barcodes.csv", f"out_{mode}"))
    shutil.rmtree(out, ignore_errors=True)
    tm = {}
    t = time.perf_counter()
    bdx.execute_demultiplexing(fq, bc, out, max_error_rate=0.1, _io=mode, _timings=tm)
    dt = time.perf_counter() - t
    nb = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    assert nb == n * 319, (nb, n * 319)
    shutil.rmtree(out, ignore_errors=True)
    tm = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in tm.items()}
    print("RESULT " + json.dumps({"mode": mode, "seconds": round(dt, 4), "reads_per_s": n / dt, "stages": tm}), flush=True)


def main() -> None:
    n = int(os.environ.get("N", "10000000"))
    reps = int(os.environ.get("REPS", "3"))
    root = os.environ.get("E2E_ROOT") or "/dev/shm/bdx_e2e_device_probe"
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    make_input(root, n)
    gen_s = time.perf_counter() - t0
    env = dict(os.environ, E2E_ROOT=root, N=str(n))
    runs = []
    try:
        for rep in range(reps):
            for mode in ("native", "device"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env, capture_output=True,
                                   text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"{mode} run {rep} failed (rc {p.returncode})")
                r = json.loads(line[0][7:])
                r["rep"] = rep
                runs.append(r)
                st = r["stages"]
                keys = ("index_s", "pack_s", "classify_s", "write_s") if mode == "native" else ("upload_s", "device_s", "download_s", "write_s")
                print(f"RUN {rep} {mode:6s} {r['seconds']:.4f} s  {r['reads_per_s'] / 1e6:6.1f} M reads/s  "
                      + "  ".join(f"{k} {st.get(k, 0):.4f}" for k in keys) + f"  batches {st.get('batches')}", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    summary = {"reads": n, "fastq_gb": n * 319 / 1e9, "where": root, "generate_s": round(gen_s, 2), "runs": runs}
    for mode in ("native", "device"):
        rs = [r for r in runs if r["mode"] == mode]
        med = statistics.median(r["reads_per_s"] for r in rs)
        stages = {k: statistics.median(r["stages"][k] for r in rs) for k in rs[0]["stages"] if isinstance(rs[0]["stages"][k], (int, float))}
        summary[mode] = {"median_reads_per_s": med, "median_stage_s": stages}
        print(f"MEDIAN {mode:6s} {med / 1e6:.1f} M reads/s  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(stages.items())))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
