"""What the penalties (repetition / presence / frequency, include/zgml_hip.h) cost in the sampled resident loop, and that a call
without them costs what it did: µs per token of
    penalised     zgml_hip_resident_decode_sampled with repeat_penalty 1.1 over the last 64 tokens (llama.cpp's defaults)
    penalised_256 ... with all three penalties over the last 256 tokens (the largest window: the counting is O(W^2))
    plain         the same loop without penalties, this build
    parent        the same loop of ANOTHER build of the library — the parent commit's, given as argv[4] — on a context and a
                  program of its own over the same weights
all in one process, alternating inside every repetition, one untimed run of each first (graph capture). One JSON line; every
repetition's figure is kept, `spread_us` is the largest difference between two repetitions of one variant.

    timeout -k 10 300 python tools/penalty_decode_run.py smollm-135m 200 5 /path/to/parent/libzgml_hip.so

    argv: preset [steps = 200] [reps = 5] [parent library = none] [start position = 8]

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it. Checked as well: plain and parent give the same tokens, and neutral penalties with a
window give them too."""
import ctypes as C
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402

arg = lambda i, default, kind: kind(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
name = arg(1, "smollm-135m", str)
steps, reps, parent, start = arg(2, 200, int), arg(3, 5, int), arg(4, "", str), arg(5, 8, int)

libs = {"this": capi.load_hip()}
if parent:
    libs["parent"] = C.CDLL(parent)
    capi._bind_hip(libs["parent"])


def use(which):  # (the Python wrappers ask capi.load_hip() at every call)
    capi._hip_lib = libs[which]


cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
assert start + steps <= cfg.max_seq_len
m = llama.Model(cfg, llama.Q4_0, threads=16)
side, history = {}, None
for which in libs:
    use(which)
    be = Backend(0)
    s = llama.Session(m, llama.hip_backend_fns(be))
    s.resident_setup(be)
    warm = s.resident_decode(1, 0, start).tolist() if start else []  # warm-up, and the cache behind the start position
    assert history in (None, [1] + warm[:-1])
    history, first = [1] + warm[:-1], (warm[-1] if start else 1)  # the tokens at positions 0 .. start - 1
    side[which] = (be, s)

base = dict(temperature=0.8, top_k=40, top_p=0.95, seed=1)
S = capi.SamplingC.of
sps = {"penalised": S(**base, repeat_penalty=1.1, penalty_window=64, recent=history),
       "penalised_256": S(**base, repeat_penalty=1.1, presence_penalty=0.25, frequency_penalty=0.25, penalty_window=256, recent=history),
       "plain": S(**base)}


def run(which, sp):
    use(which)
    return side[which][1].resident_decode_sampled(first, start, steps, sp)[0].tolist()


variants = {k: (lambda sp=sp: run("this", sp)) for k, sp in sps.items()}
if parent:
    variants["parent"] = lambda: run("parent", sps["plain"])
secs, toks = {k: [] for k in variants}, {}
for rep in range(reps + 1):  # (rep 0: untimed)
    for k, fn in variants.items():
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        assert toks.setdefault(k, out) == out, k + ": a repetition produced other tokens"
        if rep:
            secs[k].append(dt)
neutral = run("this", S(**base, repeat_penalty=1.0, penalty_window=64, recent=history))
for which, (be, _) in side.items():
    assert not be.last_error(), be.last_error()
assert neutral == toks["plain"], "neutral penalties changed the stream"
assert not parent or toks["parent"] == toks["plain"], "this build's unpenalised stream is not the parent's"
us = {k: [round(1e6 * dt / steps, 2) for dt in v] for k, v in secs.items()}
print(json.dumps({"model": name, "steps": steps, "start": start, "reps": reps, **base, "us_per_token": us,
                  "best_us": {k: min(v) for k, v in us.items()}, "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
                  "penalised_more_us": round(min(us["penalised"]) - min(us["plain"]), 2),
                  "penalised_256_more_us": round(min(us["penalised_256"]) - min(us["plain"]), 2),
                  "plain_minus_parent_us": round(min(us["plain"]) - min(us["parent"]), 2) if parent else None,
                  "penalised_differs_from_plain": toks["penalised"] != toks["plain"],
                  "distinct_tokens": {k: len(set(v)) for k, v in toks.items()}}), flush=True)
for which, (be, s) in side.items():
    use(which)
    s.close(), be.close()
m.close()
