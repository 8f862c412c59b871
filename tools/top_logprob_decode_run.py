"""What the alternatives (the `top_logprobs` word of zgml_sampling, include/zgml_hip.h) cost in the sampled resident loop, and that a
call without them costs what it did: µs per token of
    logprobs      zgml_hip_resident_decode_sampled with `logprobs` alone: [partial] .. [finish]
    top5, top64   ... with top_logprobs = 5 / 64: [finish + top] in the place of [finish], no launch more (top_logprob.hip)
    pen_logprobs  `logprobs` alone under penalties (repeat 1.3, W = 64): the penalised select, [finish]
    pen_top5, pen_top64   ... with the word: one launch more, the select over the raw row, then [finish + top]
    plain         the loop with both words 0, this build
    parent        the same loop of ANOTHER build of the library — the parent commit's, given as argv[4] — on a context and a
                  program of its own over the same weights
all in one process, alternating inside every repetition, one untimed run of each first (graph capture). One JSON line; every
repetition's figure is kept, `spread_us` is the largest difference between two repetitions of one variant.

    timeout -k 10 600 python tools/top_logprob_decode_run.py smollm-135m 200 5 /path/to/parent/libzgml_hip.so

    argv: preset [steps = 200] [reps = 5] [parent library = none] [start position = 8] [parent-first]

(parent-first: the parent build's context and program are created before this build's — two contexts of one process have measured
a few µs apart on identical code, DESIGN section 4.14, so the comparison is run both ways round.)

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens, the
values and the alternatives on the host; the clock is the host's around it, so the getter's copies are inside. Checked as well: the
word changes neither the tokens nor the values, this build's plain stream is the parent's, and alternative 0 of every token has
the largest value of its row of alternatives."""
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
parent_first = arg(6, "", str) == "parent-first"

libs = {"this": capi.load_hip()}
if parent:
    libs["parent"] = C.CDLL(parent)
    capi._bind_hip(libs["parent"])
    if parent_first:
        libs = {"parent": libs["parent"], "this": libs["this"]}


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

base = dict(temperature=0.8, top_k=40, top_p=0.95, seed=1)
sp = capi.SamplingC.of(**base)  # (to an older build the two words are the padding they were)
sp_pen = capi.SamplingC.of(**base, repeat_penalty=1.3, penalty_window=64)
kept = {}


def run(which, sampling, logprobs=False, top=0, key=None):
    use(which)
    out = side[which][1].resident_decode_sampled(first, start, steps, sampling, logprobs=logprobs, **({"top_logprobs": top} if top else {}))
    if key:
        kept[key] = out[2:]
    return out[0].tolist()


variants = {"logprobs": lambda: run("this", sp, True, key="logprobs"), "top5": lambda: run("this", sp, True, 5, "top5"),
            "top64": lambda: run("this", sp, True, 64, "top64"), "pen_logprobs": lambda: run("this", sp_pen, True, key="pen_logprobs"),
            "pen_top5": lambda: run("this", sp_pen, True, 5, "pen_top5"), "pen_top64": lambda: run("this", sp_pen, True, 64, "pen_top64"),
            "plain": lambda: run("this", sp)}
if parent:
    variants["parent"] = lambda: run("parent", sp)
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
assert toks["logprobs"] == toks["plain"] == toks["top5"] == toks["top64"], "the word changed the stream"
assert toks["pen_logprobs"] == toks["pen_top5"] == toks["pen_top64"], "the word changed the penalised stream"
assert not parent or toks["parent"] == toks["plain"], "this build's stream is not the parent's"
for a, b in (("logprobs", "top5"), ("logprobs", "top64"), ("pen_logprobs", "pen_top5"), ("pen_logprobs", "pen_top64")):
    assert np.array_equal(kept[a][0].view(np.uint32), kept[b][0].view(np.uint32)), b + ": the word changed the values"
for k, width in (("top5", 5), ("top64", 64), ("pen_top5", 5), ("pen_top64", 64)):
    alt, val = kept[k][1]
    assert alt.shape == (steps, width) and np.all(alt >= 0) and np.all(val[:, 1:] <= val[:, :-1]), k
    chosen = kept[k][0]
    assert np.all(chosen <= val[:, 0])  # no token's value lies above alternative 0's
us = {k: [round(1e6 * dt / steps, 2) for dt in v] for k, v in secs.items()}
best = {k: min(v) for k, v in us.items()}
print(json.dumps({"model": name, "steps": steps, "start": start, "reps": reps, "created_first": next(iter(libs)), "us_per_token": us, "best_us": best,
                  "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
                  "top5_more_than_logprobs_us": round(best["top5"] - best["logprobs"], 2), "top64_more_than_logprobs_us": round(best["top64"] - best["logprobs"], 2),
                  "pen_top5_more_than_pen_logprobs_us": round(best["pen_top5"] - best["pen_logprobs"], 2),
                  "pen_top64_more_than_pen_logprobs_us": round(best["pen_top64"] - best["pen_logprobs"], 2),
                  "plain_minus_parent_us": round(best["plain"] - best["parent"], 2) if parent else None,
                  "distinct_tokens": len(set(toks["plain"]))}), flush=True)
for which, (be, s) in side.items():
    use(which)
    s.close(), be.close()
m.close()
