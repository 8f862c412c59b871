#!/usr/bin/env python3
"""A/B of the Llama-2-7B Q4_0 prefill chunk time between builds of the HIP library, in one session.

    tools/prefill_chunk_ab.py parent=/path/to/other/libzgml_hip.so fix=zgml_amd/lib/libzgml_hip.so [--runs 3] [--chunks 32:8,128:4]

The libraries alternate (parent, fix, parent, fix, ...), each run in a fresh process that loads its library through ZGML_HIP_LIB and
runs bench.py's own prefill legs (prefill_leg: fixture parity first, then resident replays of the chunk's program) for chunks of 32
and of 128 tokens (--chunks tokens:timed replays; the default is what bench.py's Llama-2-7B leg passes to prefill_leg). Prints one
RESULT line per run with the seconds it took, then the median and range per library; stops at the first run that fails."""
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHUNKS = "32:8,128:4"
RUN_TIMEOUT = 120  # a run took 6-7 s on an MI355X (profiles/r09_attn_skip_prefill_ab.txt)


def chunks_of(text):
    return [tuple(int(x) for x in c.split(":")) for c in text.split(",")]


def leg(chunks):
    sys.path.insert(0, str(ROOT))
    import bench
    from zgml_amd import Backend, llama
    be = Backend(0)
    out = {}
    for T, reps in chunks:
        r = bench.prefill_leg(be, llama, "q4_0", T=T, reps=reps)
        out[f"prefill{T}_ms_per_chunk"] = r["ms_per_chunk"]
        out[f"prefill{T}_verified"] = r["verified"]
    be.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    chunks = args[args.index("--chunks") + 1] if "--chunks" in args else CHUNKS
    if "--leg" in args:
        return leg(chunks_of(chunks))
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 3
    libs = [a.split("=", 1) for a in args if "=" in a]
    got = {name: [] for name, _ in libs}
    for i in range(runs):
        for name, path in libs:
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, __file__, "--leg", "--chunks", chunks], capture_output=True, text=True, timeout=RUN_TIMEOUT,
                               env=dict(os.environ, ZGML_HIP_LIB=str(Path(path).resolve())))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit(f"run {i + 1} {name} failed (rc {r.returncode}):\n{r.stdout[-1500:]}{r.stderr[-1500:]}")
            print(f"== run {i + 1} {name} ({time.perf_counter() - t0:.0f} s)\n{line[-1]}", flush=True)
            got[name].append(json.loads(line[-1][len("RESULT "):]))
    for T, _ in chunks_of(chunks):
        for name, _ in libs:
            v = [g[f"prefill{T}_ms_per_chunk"] for g in got[name]]
            print(f"prefill{T} {name}: median {statistics.median(v):.3f} ms, range {min(v):.3f}..{max(v):.3f}")


if __name__ == "__main__":
    main()
