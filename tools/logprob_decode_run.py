"""What the log-probabilities (the `logprobs` field of zgml_sampling, include/zgml_hip.h) cost in the sampled resident loop, and that
a call without them costs what it did: µs per token of
    logprobs      zgml_hip_resident_decode_sampled with the field set: two launches more per token ([partial] [finish], logprob.hip)
    plain         the same loop without the field, this build
    parent        the same loop of ANOTHER build of the library — the parent commit's, given as argv[4] — on a context and a
                  program of its own over the same weights
all in one process, alternating inside every repetition, one untimed run of each first (graph capture). One JSON line; every
repetition's figure is kept, `spread_us` is the largest difference between two repetitions of one variant.

    timeout -k 10 300 python tools/logprob_decode_run.py smollm-135m 200 5 /path/to/parent/libzgml_hip.so

    argv: preset [steps = 200] [reps = 5] [parent library = none] [start position = 8]

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens (and
the values) on the host; the clock is the host's around it. Checked as well: the three variants give the same tokens, and the
values are finite and not positive."""
import ctypes as C
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
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
side, first = {}, 1
for which in libs:
    use(which)
    be = Backend(0)
    s = llama.Session(m, llama.hip_backend_fns(be))
    s.resident_setup(be)
    warm = s.resident_decode(1, 0, start).tolist() if start else []  # warm-up, and the cache behind the start position
    first = warm[-1] if start else 1
    side[which] = (be, s)

sp = capi.SamplingC.of(temperature=0.8, top_k=40, top_p=0.95, seed=1)  # (to an older build the `logprobs` word is the padding it was)
values = {}


def run(which, logprobs):
    use(which)
    out = side[which][1].resident_decode_sampled(first, start, steps, sp, logprobs=logprobs)
    if logprobs:
        values["logprobs"] = out[2]
    return out[0].tolist()


variants = {"logprobs": lambda: run("this", True), "plain": lambda: run("this", False)}
if parent:
    variants["parent"] = lambda: run("parent", False)
secs, toks = {k: [] for k in variants}, {}
for rep in range(reps + 1):  # (rep 0: untimed)
    for k, fn in variants.items():
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        assert toks.setdefault(k, out) == out, k + ": a repetition produced other tokens"
        if rep:
            secs[k].append(dt)
for which, (be, _) in side.items():
    assert not be.last_error(), be.last_error()
assert toks["logprobs"] == toks["plain"], "the field changed the stream"
assert not parent or toks["parent"] == toks["plain"], "this build's stream is not the parent's"
lp = values["logprobs"]
assert np.all(np.isfinite(lp)) and np.all(lp <= 0)
us = {k: [round(1e6 * dt / steps, 2) for dt in v] for k, v in secs.items()}
print(json.dumps({"model": name, "steps": steps, "start": start, "reps": reps, "us_per_token": us,
                  "best_us": {k: min(v) for k, v in us.items()}, "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
                  "logprobs_more_us": round(min(us["logprobs"]) - min(us["plain"]), 2),
                  "plain_minus_parent_us": round(min(us["plain"]) - min(us["parent"]), 2) if parent else None,
                  "mean_logprob": round(float(lp.mean()), 4), "distinct_tokens": len(set(toks["plain"]))}), flush=True)
for which, (be, s) in side.items():
    use(which)
    s.close(), be.close()
m.close()
