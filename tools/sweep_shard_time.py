#!/usr/bin/env python
"""WHDR sweep as a command, one process against two ranks on the one device: what the process group
and the gather cost.

The 64 photos of tools/sweep_load_time.py (341x512 and 512x341 alternating, every 16th 384x512, a
judgement file beside each) and one pair, bilateral sigma_color 20 sigma_spatial 22.  Timed is the
command, from its start to its end with the JSON written:
    world 1   python -m reflectance_filtering_amd.sweep ...                    the parent commit's behaviour
    world 2   the same under RANK / WORLD_SIZE / LOCAL_RANK, both ranks on device 0, 32 photos each
After one warm-up each, --reps alternating repeats (world 1, world 2, world 1, ...): median and
min-max per world size.  The two JSON files are asserted equal, byte for byte.

Two ranks on one device share the device and the CPUs of the machine, so this measures the overhead
of the group and the gather, not scaling; the curve over real devices is not measured here.

Every rank is a child process under a time limit of its own; a rank that ends non-zero ends the
tool (the other rank is killed, nothing is started again).  Prints a table on stdout and one JSON
line last; --out also writes the table to a file.

    python tools/sweep_shard_time.py [--n 64] [--points 300] [--reps 5] [--out profiles/sweep_shard_time.txt]
"""
import argparse
import json
import os
import shutil
import signal
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANK_SECONDS = 240
RANK_KEYS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def command(photos_glob, out, world):
    """One run of the sweep at `world` ranks: seconds from the start of the first rank to the end of
    the last."""
    env = {k: v for k, v in os.environ.items() if k not in RANK_KEYS}
    cmd = ["timeout", "-k", "10", str(RANK_SECONDS), sys.executable, "-m", "reflectance_filtering_amd.sweep",
           "--inputs", photos_glob, "--filter_type", "bilateral", "--sigma_color", "20", "--sigma_spatial",
           "22", "--out", out, "--group_timeout", "120"]
    port = free_port()
    t0 = time.perf_counter()
    procs = []
    for rank in range(world):
        extra = {} if world == 1 else dict(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                                           LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                           MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, cwd=ROOT, env=dict(env, **extra), stdout=subprocess.DEVNULL,
                                      start_new_session=True))
    try:
        for rank, p in enumerate(procs):
            code = p.wait(timeout=RANK_SECONDS + 30)
            if code != 0:
                raise SystemExit("rank %d of %d ended with %d: stopping" % (rank, world, code))
    finally:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--points", type=int, default=300, help="distinct judgement points per image")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    from tools.sweep_load_time import write_inputs
    work = tempfile.mkdtemp(prefix="sweep_shard_time_")
    worlds = (1, 2)
    times = {w: [] for w in worlds}
    try:
        write_inputs(work, args.n, args.points)
        photos_glob = os.path.join(work, "photos", "*.png")
        outs = {w: os.path.join(work, "sweep_w%d.json" % w) for w in worlds}
        for w in worlds:                        # warm-up: file cache, code object cache
            command(photos_glob, outs[w], w)
        for _ in range(args.reps):
            for w in worlds:
                os.remove(outs[w])
                times[w].append(command(photos_glob, outs[w], w))
        texts = {}
        for w in worlds:
            with open(outs[w], "rb") as fh:
                texts[w] = fh.read()
        assert texts[1] == texts[2], "two ranks wrote another JSON than one process"
    finally:
        shutil.rmtree(work, ignore_errors=True)
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    lines = ["sweep as a command, %d photos, bilateral c20 s22, %d judgement points each; %d CPUs in the "
             "affinity mask" % (args.n, args.points, cpus),
             "seconds from the start of the command to its end (JSON written), %d alternating repeats "
             "after one warm-up each" % args.reps]
    line = {"tool": "sweep_shard_time", "n": args.n, "points_per_image": args.points, "reps": args.reps,
            "cpus": cpus, "json_equal": True, "worlds": {}}
    for w in worlds:
        ts = times[w]
        lines.append("    world %d (%s)   median %7.3f s   min %7.3f   max %7.3f"
                     % (w, "one process" if w == 1 else "two ranks on device 0", statistics.median(ts),
                        min(ts), max(ts)))
        line["worlds"][str(w)] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                                  "seconds": ts}
    apart = max(times[2]) < min(times[1]) or max(times[1]) < min(times[2])
    lines.append("the ranges %s" % ("do not touch" if apart else "touch: no difference is claimed"))
    lines.append("the two JSON files are equal byte for byte")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
