"""The sampled resident loop (zgml_hip_resident_decode_sampled) against the greedy resident loop of the same build, same plan and
same process: tok/s of both, alternating inside every repetition, one untimed run of each first (graph capture) behind the
warm-up of bench.py's resident legs. One JSON line; every repetition's figure is kept.

    timeout -k 10 300 python tools/sampled_decode_run.py smollm-135m && timeout -k 10 900 python tools/sampled_decode_run.py llama2-7b

    argv: preset [steps = 200] [reps = 3] [temperature = 0.8] [top_k = 40] [top_p = 0.95] [seed = 1] [start position = 8]

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it. The sampled tokens are also checked: top_k = 1 must reproduce the greedy tokens."""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402

arg = lambda i, default, kind: kind(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
name = arg(1, "smollm-135m", str)
steps, reps = arg(2, 200, int), arg(3, 3, int)
temperature, top_k, top_p, seed, start = arg(4, 0.8, float), arg(5, 40, int), arg(6, 0.95, float), arg(7, 1, int), arg(8, 8, int)

be = Backend(0)
cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
assert start + steps <= cfg.max_seq_len
m = llama.Model(cfg, llama.Q4_0, threads=16)
s = llama.Session(m, llama.hip_backend_fns(be))
s.resident_setup(be)
first = int(s.resident_decode(1, 0, start)[-1]) if start else 1  # warm-up, and the cache behind the start position
sp = capi.SamplingC.of(temperature, top_k, top_p, seed=seed)
variants = {"greedy": lambda: s.resident_decode(first, start, steps),
            "sampled": lambda: s.resident_decode_sampled(first, start, steps, sp)[0]}
secs = {k: [] for k in variants}
toks = {}
for rep in range(reps + 1):  # (rep 0: untimed)
    for k, run in variants.items():
        t0 = time.perf_counter()
        out = run().tolist()
        dt = time.perf_counter() - t0
        assert toks.setdefault(k, out) == out, k + ": a repetition produced other tokens"
        if rep:
            secs[k].append(dt)
k1 = s.resident_decode_sampled(first, start, steps, capi.SamplingC.of(temperature, 1, top_p, seed=seed))[0].tolist()
assert not be.last_error(), be.last_error()
assert k1 == toks["greedy"], "top_k = 1 is not the greedy stream"
tok_s = {k: [round(steps / dt, 1) for dt in v] for k, v in secs.items()}
print(json.dumps({"model": name, "steps": steps, "start": start, "temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed,
                  "launches_per_token": be.planText(s.handle).count("\n") + 3, "greedy_tok_s": tok_s["greedy"], "sampled_tok_s": tok_s["sampled"],
                  "sampled_over_greedy": round(max(tok_s["sampled"]) / max(tok_s["greedy"]), 4),
                  "us_per_token_more": round(1e6 * (min(secs["sampled"]) - min(secs["greedy"])) / steps, 2),
                  "distinct_sampled_tokens": len(set(toks["sampled"]))}), flush=True)
s.close(), m.close(), be.close()
