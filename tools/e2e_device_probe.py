#!/usr/bin/env python3
"""End-to-end reads/s of execute_demultiplexing on the C2 shape: the native host pipeline (_io="native") against the device
FASTQ pipeline (_io="device"), each run in a fresh child process (GPU box).

  N=10000000 REPS=3 python tools/e2e_device_probe.py [--gzip {host,device} [--gzip-level 2] | --gunzip | --gunzip-stream | --gunzip-window | --deal | --check] [out.json]

One synthetic FASTQ of N 150 bp reads x 96 barcodes (24 bp), max_error_rate=0.1, on tmpfs (/dev/shm unless E2E_ROOT is
set); the outputs are checked (total bytes = input bytes).  Prints every run with its stage seconds, then the medians; the
optional argument receives the same as JSON.

--gzip host: both legs write gzip (gzip_output=True, zlib on the host threads): "native+gz" and "device+gz".  --gzip device
adds the leg "device+dgz" (_gzip="device": DEFLATE on the GPU) to the same alternating series, and with --gzip-level 2
the leg "device+dgz2" (_gzip_level=2) as well.  The check then sums the ISIZE fields along the members' size tags.  Every
leg reports min, median and max wall seconds.

--gunzip: .gz in -> .gz out through the device pipeline only.  The input is written once as 32 KiB 'D','X' members (zlib
level 1 on host threads) and three legs alternate after one unrecorded warm-up run: "device+gz+hin" (host inflate, host
gzip), "device+dgz+hin" (host inflate, device gzip) and "device+dgz+din" (_gunzip="device": inflate on the GPU, device
gzip).

--gunzip-stream: an ORDINARY .gz in -> plain out through the device pipeline.  The input is written once as ONE gzip member
(zlib level 6; slices compressed side by side and joined with sync flushes, as pigz does) and two legs alternate after one
unrecorded warm-up run: "device++hsin" (_gunzip="host": one zlib thread) and "device++sin" (_gunzip="device-stream").
Before that, one run of the stream leg per chunk size of 16, 32, 64 and 128 KiB ("sweep").  REPS=5 is what the
repository's figures use; every leg reports min, median and max wall seconds and the plain GB/s they amount to.

--gunzip-window: the same input and the same two legs, and a third, "device++win" (_gunzip="device-window").  Before the
series, one run of the windowed leg per window size of 16, 64 and 256 MiB (2^28 bytes, the largest) ("sweep"); the series
then runs the windowed leg at the sweep's fastest size (E2E_WINDOW overrides it), which is reported as "window_bytes".  The
stream and windowed legs also report "device_peak_bytes": the largest drop of the device's free memory (hipMemGetInfo, sampled
every 10 ms by a thread of the child; other processes on the device would show in it too) below its value at the start.

--deal: plain in -> plain out; four legs alternate after one unrecorded warm-up run: "device" (_io="device", the baseline)
and "deal1", "deal2", "deal3" (_io="device-deal" with devices=[0], [0, 0] and [0, 0, 0]: one, two and three contexts on
GPU 0, the default span).  REPS=5 is what the repository's figures use; every leg reports min, median and max wall seconds.

--check: what the opt-in checks (_check=True) cost; plain in -> plain out through _io="device".  Legs "device" (_check
off) and "device-chk" (on), single-end, and "pair" / "pair-chk" for a paired run (R2: the same headers, the sequences
reversed; only R2 is written).  With E2E_PARENT naming a built checkout of the commit to compare against, the legs "parent"
and "parent-pair" run the same calls with THAT checkout's package: the off legs are judged against them.  All legs alternate
after one unrecorded warm-up run; the checked legs also report check_s."""
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


def make_gz_input(root: str, member: int = 32768) -> None:
    """synthetic.fastq.gz beside synthetic.fastq: a chain of 'D','X'-tagged members of `member` plain bytes"""
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    fq = os.path.join(root, "synthetic.fastq")
    if os.path.exists(fq + ".gz"):
        return
    d = np.memmap(fq, dtype=np.uint8, mode="r")

    def one(o):
        part = bytes(d[o:o + member])
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = z.compress(part) + z.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x08\0DX\x04\0" + (len(body) + 28).to_bytes(4, "little") + body
                + zlib.crc32(part).to_bytes(4, "little") + len(part).to_bytes(4, "little"))

    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex, open(fq + ".gz", "wb") as f:
        for m in ex.map(one, range(0, len(d), member)):
            f.write(m)


def make_stream_gz_input(root: str, slices: int = 64) -> None:
    """synthetic.stream.fastq.gz beside synthetic.fastq: one ordinary gzip member, zlib level 6"""
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    fq = os.path.join(root, "synthetic.fastq")
    if os.path.exists(fq[:-6] + ".stream.fastq.gz"):
        return
    d = np.memmap(fq, dtype=np.uint8, mode="r")
    step = -(-len(d) // slices)

    def one(k):
        part = bytes(d[k * step:(k + 1) * step])
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        return z.compress(part) + z.flush(zlib.Z_FINISH if k == slices - 1 else zlib.Z_SYNC_FLUSH), zlib.crc32(part), len(part)

    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex, open(fq[:-6] + ".stream.fastq.gz", "wb") as f:
        f.write(b"\x1f\x8b\x08\0\0\0\0\0\0\xff")
        crc = 0
        for body, c, n in ex.map(one, range(slices)):
            f.write(body)
            crc = zlib.crc32_combine(crc, c, n) if hasattr(zlib, "crc32_combine") else None
        if crc is None:
            crc = 0
            for o in range(0, len(d), 1 << 26):
                crc = zlib.crc32(d[o:o + (1 << 26)], crc)
        f.write(crc.to_bytes(4, "little") + (len(d) & 0xFFFFFFFF).to_bytes(4, "little"))


def gz_sizes(path: str):
    """(compressed, uncompressed) bytes of a file made of size-tagged gzip members"""
    import numpy as np

    d = np.memmap(path, dtype=np.uint8, mode="r")
    p, plain = 0, 0
    while p < len(d):
        assert bytes(d[p:p + 4]) == b"\x1f\x8b\x08\x04" and bytes(d[p + 12:p + 14]) == b"DX", (path, p)
        p += int.from_bytes(bytes(d[p + 16:p + 20]), "little")
        plain += int.from_bytes(bytes(d[p - 4:p]), "little")
    assert p == len(d), (path, p, len(d))
    return len(d), plain


class FreeMemory:
    """samples the device's free memory from a thread of its own; stop() -> the largest drop below the first sample"""

    def __init__(self, period: float = 0.01):
        import ctypes as C
        import threading

        from biodemux_jl_amd.hipabi import load_library

        lib = load_library()
        lib.hipMemGetInfo.restype = C.c_int
        lib.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        self.done = threading.Event()

        def free():
            f, t = C.c_size_t(0), C.c_size_t(0)
            return f.value if lib.hipMemGetInfo(C.byref(f), C.byref(t)) == 0 else None

        self.first = self.low = free()

        def loop():
            while not self.done.wait(period):
                f = free()
                if f is not None and self.low is not None:
                    self.low = min(self.low, f)

        self.thread = threading.Thread(target=loop, name="bdx-probe-free-memory", daemon=True)
        self.thread.start()

    def stop(self):
        self.done.set()
        self.thread.join()
        return None if self.first is None else int(self.first - self.low)


CHECK_LEGS = ("device", "device-chk", "pair", "pair-chk")
PARENT_LEGS = ("parent", "parent-pair")


def make_pair_input(root: str, n: int) -> None:
    """synthetic_R2.fastq beside synthetic.fastq: the same records with every sequence reversed"""
    import numpy as np

    fq = os.path.join(root, "synthetic_R2.fastq")
    if os.path.exists(fq) and os.path.getsize(fq) == n * 319:
        return
    rec = np.fromfile(os.path.join(root, "synthetic.fastq"), dtype=np.uint8).reshape(n, 319)
    rec[:, 15:165] = rec[:, 164:14:-1]
    rec.tofile(fq)


def child(mode: str) -> None:
    if mode in PARENT_LEGS:  # the package of the checkout to compare against
        sys.path.insert(0, os.environ["E2E_PARENT"])
    import biodemux_jl_amd as bdx

    root = os.environ["E2E_ROOT"]
    n = int(os.environ["N"])
    io, gz, gin = (mode.split("+") + ["", ""])[:3]
    fq, bc, out = (os.path.join(root, x) for x in ("synthetic.fastq", "barcodes.csv", f"out_{io}_{gz}_{gin}"))
    shutil.rmtree(out, ignore_errors=True)
    tm = {}
    kw = dict(gzip_output=True) if gz else {}
    fastqs = [fq]
    if mode in CHECK_LEGS[1:] + PARENT_LEGS:
        io = "device"
        if "pair" in mode:
            fastqs.append(os.path.join(root, "synthetic_R2.fastq"))
        if mode.endswith("-chk"):
            kw["_check"] = True
    if io.startswith("deal"):  # _io="device-deal" on that many contexts of GPU 0
        kw["devices"] = [0] * int(io[4:])
        io = "device-deal"
    if gz in ("dgz", "dgz2"):
        kw["_gzip"] = "device"
    if gz == "dgz2":
        kw["_gzip_level"] = 2
    sampler = None
    if gin in ("hsin", "sin", "win"):
        from biodemux_jl_amd import deviceio

        fq = fq[:-6] + ".stream.fastq.gz"
        kw.update(gzip_output=False, output_prefix="synthetic")
        if gin == "sin":
            kw["_gunzip"] = "device-stream"
            deviceio.STREAM_CHUNK = int(os.environ.get("E2E_STREAM_CHUNK", "0"))
        if gin == "win":
            kw["_gunzip"] = "device-window"
            if os.environ.get("E2E_WINDOW"):
                kw["_gunzip_window"] = int(os.environ["E2E_WINDOW"])
        if gin != "hsin":
            sampler = FreeMemory()
    elif gin:
        fq += ".gz"
    if gin == "din":
        kw["_gunzip"] = "device"
    t = time.perf_counter()
    if len(fastqs) == 1:
        fastqs = [fq]  # (the .gz legs have renamed it)
    bdx.execute_demultiplexing(*fastqs, bc, out, max_error_rate=0.1, _io=io, _timings=tm, **kw)
    dt = time.perf_counter() - t
    if sampler is not None:
        tm["device_peak_bytes"] = sampler.stop()
    files = [os.path.join(out, f) for f in os.listdir(out)]
    if gz:
        sizes = [gz_sizes(f) for f in files]
        nb = sum(s[1] for s in sizes)
        tm["file_bytes"] = sum(s[0] for s in sizes)
    else:
        nb = sum(os.path.getsize(f) for f in files)
    assert nb == n * 319, (nb, n * 319)
    shutil.rmtree(out, ignore_errors=True)
    tm = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in tm.items()}
    print("RESULT " + json.dumps({"mode": mode, "seconds": round(dt, 4), "reads_per_s": n / dt, "stages": tm}), flush=True)


def main() -> None:
    argv = sys.argv[1:]
    modes = ["native", "device"]
    if argv and argv[0] == "--gzip":
        if len(argv) < 2 or argv[1] not in ("host", "device"):
            raise SystemExit("--gzip takes host or device")
        modes = ["native+gz", "device+gz"] + (["device+dgz"] if argv[1] == "device" else [])
        argv = argv[2:]
        if argv and argv[0] == "--gzip-level":
            if modes[-1] != "device+dgz" or len(argv) < 2 or argv[1] not in ("1", "2"):
                raise SystemExit("--gzip-level takes 1 or 2 and goes with --gzip device")
            modes += ["device+dgz2"] if argv[1] == "2" else []
            argv = argv[2:]
    gunzip = bool(argv) and argv[0] == "--gunzip"
    if gunzip:
        modes = ["device+gz+hin", "device+dgz+hin", "device+dgz+din"]
        argv = argv[1:]
    stream = bool(argv) and argv[0] == "--gunzip-stream"
    if stream:
        modes = ["device++hsin", "device++sin"]
        argv = argv[1:]
    window = bool(argv) and argv[0] == "--gunzip-window"
    if window:
        stream = False
        modes = ["device++hsin", "device++sin", "device++win"]
        argv = argv[1:]
    deal = bool(argv) and argv[0] == "--deal"
    if deal:
        modes = ["device", "deal1", "deal2", "deal3"]
        argv = argv[1:]
    check = bool(argv) and argv[0] == "--check"
    if check:
        parent = bool(os.environ.get("E2E_PARENT"))
        modes = (["parent"] if parent else []) + ["device", "device-chk"] + (["parent-pair"] if parent else []) + ["pair", "pair-chk"]
        argv = argv[1:]
    n = int(os.environ.get("N", "10000000"))
    reps = int(os.environ.get("REPS", "3"))
    root = os.environ.get("E2E_ROOT") or "/dev/shm/bdx_e2e_device_probe"
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    make_input(root, n)
    gz_bytes = None
    if gunzip:
        make_gz_input(root)
        gz_bytes = os.path.getsize(os.path.join(root, "synthetic.fastq.gz"))
    if stream or window:
        make_stream_gz_input(root)
        gz_bytes = os.path.getsize(os.path.join(root, "synthetic.stream.fastq.gz"))
    if check:
        make_pair_input(root, n)
    gen_s = time.perf_counter() - t0
    env = dict(os.environ, E2E_ROOT=root, N=str(n))
    runs = []
    sweep = []
    try:
        for kib in (16, 32, 64, 128) if stream else ():  # one run per chunk size
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "device++sin"],
                               env=dict(env, E2E_STREAM_CHUNK=str(kib * 1024)), capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"sweep run at {kib} KiB failed (rc {p.returncode})")
            r = json.loads(line[0][7:])
            sweep.append({"chunk_kib": kib, "seconds": r["seconds"], "inflate_s": r["stages"].get("inflate_s"), "stages": r["stages"]})
            print(f"SWEEP chunk {kib:4d} KiB  {r['seconds']:.4f} s  inflate_s {r['stages'].get('inflate_s')}", flush=True)
        for mib in (16, 64, 256) if window else ():  # one run per window size
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "device++win"],
                               env=dict(env, E2E_WINDOW=str(mib << 20)), capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"sweep run at {mib} MiB failed (rc {p.returncode})")
            r = json.loads(line[0][7:])
            sweep.append({"window_mib": mib, "seconds": r["seconds"], "inflate_s": r["stages"].get("inflate_s"), "stages": r["stages"]})
            print(f"SWEEP window {mib:4d} MiB  {r['seconds']:.4f} s  inflate_s {r['stages'].get('inflate_s')}  windows "
                  f"{r['stages'].get('stream_windows')}  text peak {r['stages'].get('stream_text_peak_bytes')}  device peak "
                  f"{r['stages'].get('device_peak_bytes')}", flush=True)
        if window:
            best = int(os.environ.get("E2E_WINDOW") or min(sweep, key=lambda x: x["seconds"])["window_mib"] << 20)
            env["E2E_WINDOW"] = str(best)
            print(f"SERIES window {best} bytes", flush=True)
        for rep in range(-1 if gunzip or stream or window or deal or check else 0, reps):  # (rep -1: the warm-up run, not recorded)
            for mode in modes[:1] if rep < 0 else modes:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env, capture_output=True,
                                   text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"{mode} run {rep} failed (rc {p.returncode})")
                r = json.loads(line[0][7:])
                r["rep"] = rep
                if rep < 0:
                    continue
                runs.append(r)
                st = r["stages"]
                keys = ("index_s", "pack_s", "classify_s", "write_s") if mode.startswith("native") else ("upload_s", "device_s", "download_s", "write_s")
                if "+dgz" in mode:
                    keys += ("deflate_s",)
                if mode.endswith(("+din", "+sin", "+win")):
                    keys += ("inflate_s", "compressed_in_bytes", "plain_in_bytes")
                if mode.startswith("deal"):
                    keys += ("phase_wait_s", "spans")
                if mode.endswith("-chk"):
                    keys += ("check_s",)
                print(f"RUN {rep} {mode:10s} {r['seconds']:.4f} s  {r['reads_per_s'] / 1e6:6.1f} M reads/s  "
                      + "  ".join(f"{k} {st.get(k, 0):.4f}" for k in keys) + f"  batches {st.get('batches')}", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    summary = {"reads": n, "fastq_gb": n * 319 / 1e9, "where": root, "generate_s": round(gen_s, 2), "runs": runs}
    if gz_bytes is not None:
        summary["input_gz_bytes"] = gz_bytes
    if stream:
        summary["chunk_sweep"] = sweep
    if window:
        summary["window_sweep"] = sweep
        summary["window_bytes"] = int(env["E2E_WINDOW"])
    for mode in modes:
        rs = [r for r in runs if r["mode"] == mode]
        med = statistics.median(r["reads_per_s"] for r in rs)
        secs = sorted(r["seconds"] for r in rs)
        stages = {k: statistics.median(r["stages"][k] for r in rs) for k in rs[0]["stages"] if isinstance(rs[0]["stages"][k], (int, float))}
        summary[mode] = {"median_reads_per_s": med, "median_stage_s": stages, "seconds_min_median_max": [secs[0], statistics.median(secs), secs[-1]]}
        if stream or window:  # the leg's plain text per wall second (the host leg: what one zlib thread sustains under the pipeline)
            summary[mode]["plain_gb_per_s_min_median_max"] = [n * 319 / 1e9 / x for x in (secs[-1], statistics.median(secs), secs[0])]
        print(f"MEDIAN {mode:10s} {med / 1e6:.1f} M reads/s  wall s min {secs[0]:.4f} median {statistics.median(secs):.4f} max {secs[-1]:.4f}  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(stages.items())))
    if argv:
        with open(argv[0], "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
