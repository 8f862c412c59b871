"""Speculative resident decode of one model (zgml_hip_resident_decode_speculative) against the plain resident decode of the
token_len = 1 plan, in one process: per T the cost of a verify step, its launch count, and tokens per step / tok/s for perfect
provided drafts (upper bound T tokens per step), useless drafts (lower bound 1: this prices the overhead) and n-gram drafting on
the model's own greedy continuation of the prompt (7 i + 3) mod vocab. One JSON line per (model, T, option); every repetition's
figure is kept. The variants alternate inside each repetition; one untimed run of each comes first (graph capture), behind the
warm-up of bench.py's resident legs.

    timeout -k 10 300 python tools/spec_decode_run.py smollm-135m && timeout -k 10 900 python tools/spec_decode_run.py llama2-7b

    argv: model [T list = 2,3,4,6] [reps = 3] [small-M option list; default 1 for llama2-7b, 0,1 for the others] [prompt = 128] [generate = 256]
          [sampling = temperature,top_k,top_p,seed; default none]

With a sampling parameter set (say 0.8,40,0.95,1) the sampled entry point (zgml_hip_resident_decode_speculative_sampled) runs
beside the greedy one on the same program in the same process, its variants alternating with the greedy ones inside every
repetition: the lines then carry a "sampled" record — ms per sampled verify step, what it costs over the greedy step, and its
break-even against the plain SAMPLED loop of the decode plan (zgml_hip_resident_decode_sampled, timed beside the plain greedy one)
— and whether every sampled run gave the untimed n-gram run's tokens ("one_stream_whatever_the_drafts": the same drafts always do;
other drafts may part at a pick that turns on the last bit of the logits, include/zgml_hip.h).

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it. break_even = ms per verify step / ms per token of the plain loop: the tokens a step
must yield on average for speculation to pay."""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "smollm-135m"
Ts = [int(t) for t in sys.argv[2].split(",")] if len(sys.argv) > 2 else [2, 3, 4, 6]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
options = [int(o) for o in sys.argv[4].split(",")] if len(sys.argv) > 4 else ([1] if name == "llama2-7b" else [0, 1])
P = int(sys.argv[5]) if len(sys.argv) > 5 else 128
G = int(sys.argv[6]) if len(sys.argv) > 6 else 256
sp = None
if len(sys.argv) > 7:
    t_, k_, p_, seed_ = sys.argv[7].split(",")
    sp = capi.SamplingC.of(float(t_), int(k_), float(p_), seed=int(seed_))

be = Backend(0)
cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
m = llama.Model(cfg, llama.Q4_0, threads=16)
fns = llama.hip_backend_fns(be)
prompt = [(7 * i + 3) % cfg.vocab_size for i in range(P)]
assert P + G + max(Ts) + max(Ts) <= cfg.max_seq_len


def emit(**kw):
    print(json.dumps({"model": name, "prompt": P, "generate": G, **kw}), flush=True)


# the plain resident loop of the decode plan: the stream everything is compared with, and ms per token
s = llama.Session(m, fns)
s.resident_setup(be)
s.resident_decode(1, 0, 4)  # warm-up (bench.py's resident legs)
for pos, t in enumerate(prompt):
    first, _ = s.step(t, pos, want_logits=False)  # the prompt through the vtable; the last step's token opens the continuation
n_ref = G + max(Ts)
stream = s.resident_decode(first, P, n_ref).tolist()  # (untimed: graph capture)
single = []
for _ in range(reps):
    t0 = time.perf_counter()
    again = s.resident_decode(first, P, n_ref).tolist()
    single.append((time.perf_counter() - t0) / n_ref)
    assert again == stream
assert not be.last_error(), be.last_error()
ms_tok = 1e3 * min(single)
emit(path="single", launches=be.planText(s.handle).count("\n") + 3, ms_per_token=[round(1e3 * t, 4) for t in single], tok_s=[round(1 / t, 1) for t in single])
ms_tok_sampled = None
if sp is not None:  # the plain sampled loop of the same plan: what a sampling caller has without speculation
    s.resident_decode_sampled(first, P, n_ref, sp)  # (untimed: graph capture)
    single_s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.resident_decode_sampled(first, P, n_ref, sp)
        single_s.append((time.perf_counter() - t0) / n_ref)
    assert not be.last_error(), be.last_error()
    ms_tok_sampled = 1e3 * min(single_s)
    emit(path="single_sampled", launches=be.planText(s.handle).count("\n") + 3, ms_per_token=[round(1e3 * t, 4) for t in single_s],
         tok_s=[round(1 / t, 1) for t in single_s])
s.close()

for T in Ts:
    for on in options:
        mt = llama.Model(cfg, llama.Q4_0, threads=16, token_len=T)
        be.set_option(capi.OPT_SMALL_M_MATVEC, on)
        try:
            st = llama.Session(mt, fns)
        finally:
            be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
        st.resident_setup(be)
        for pos in list(range(0, P - T + 1, T)) + ([P - T] if P % T else []):  # the prompt in chunks of T (the last one overlaps)
            st.resident_prefill(prompt[pos:pos + T], pos)
        variants = {"perfect": dict(drafts=stream), "useless": dict(drafts=[(t + 1) % cfg.vocab_size for t in stream]),
                    "ngram": dict(history=prompt)}
        runs = {k: [] for k in variants}
        variants_s, runs_s = {}, {}
        if sp is not None:
            # the sampled stream of THIS plan (its rows are the M = T kernels': the decode plan's stream may part from it) from an
            # untimed n-gram run, G + T tokens of it so that perfect drafts exist for the last step
            stream_s = st.resident_decode_speculative_sampled(first, P, G + T, sp, history=prompt)[0].tolist()
            variants_s = {"perfect": dict(drafts=stream_s), "useless": dict(drafts=[(t + 1) % cfg.vocab_size for t in stream_s]),
                          "ngram": dict(history=prompt)}
            runs_s = {k: [] for k in variants_s}
        for rep in range(reps + 1):  # (rep 0: untimed)
            for k, kw in variants.items():
                t0 = time.perf_counter()
                toks, stats = st.resident_decode_speculative(first, P, G, **kw)
                dt = time.perf_counter() - t0
                if rep:
                    runs[k].append((dt, stats, toks.tolist() == stream[:G]))
                if k in variants_s:
                    t0 = time.perf_counter()
                    toks, produced, stats = st.resident_decode_speculative_sampled(first, P, G, sp, **variants_s[k])
                    dt = time.perf_counter() - t0
                    if rep:
                        runs_s[k].append((dt, stats, produced == G and toks.tolist() == stream_s[:G]))
        assert not be.last_error(), be.last_error()
        text = be.planText(st.handle)
        out = {"path": "speculative", "T": T, "option": on, "launches_per_step": text.count("\n") + 4, "rows_kernel_launches": text.count("qmatvec-kon-rows")}
        step_ms = min(1e3 * dt / stats["steps"] for dt, stats, _ in runs["useless"])
        out["ms_per_verify_step"] = round(step_ms, 4)
        out["break_even_tokens_per_step"] = round(step_ms / ms_tok, 3)
        for k, r in runs.items():
            best = min(dt for dt, _, _ in r)
            out[k] = {"tokens_equal_plain_decode": all(eq for _, _, eq in r), "steps": r[0][1]["steps"], "drafted": r[0][1]["drafted"],
                      "accepted": r[0][1]["accepted"], "tokens_per_step": round(G / r[0][1]["steps"], 3),
                      "ms_per_step": [round(1e3 * dt / st_["steps"], 4) for dt, st_, _ in r], "tok_s": [round(G / dt, 1) for dt, _, _ in r],
                      "vs_plain": round(G / best / (1e3 / ms_tok), 3)}
        if sp is not None:
            step_ms_s = min(1e3 * dt / stats["steps"] for dt, stats, _ in runs_s["useless"])
            rec = {"sampling": sys.argv[7], "launches_per_step": text.count("\n") + 5, "ms_per_verify_step": round(step_ms_s, 4),
                   "us_per_step_over_greedy": round(1e3 * (step_ms_s - step_ms), 2),
                   "break_even_tokens_per_step": round(step_ms_s / ms_tok_sampled, 3), "break_even_vs_plain_greedy": round(step_ms_s / ms_tok, 3)}
            for k, r in runs_s.items():
                best = min(dt for dt, _, _ in r)
                rec[k] = {"one_stream_whatever_the_drafts": all(eq for _, _, eq in r), "steps": r[0][1]["steps"], "accepted": r[0][1]["accepted"],
                          "tokens_per_step": round(G / r[0][1]["steps"], 3), "ms_per_step": [round(1e3 * dt / st_["steps"], 4) for dt, st_, _ in r],
                          "tok_s": [round(G / dt, 1) for dt, _, _ in r], "vs_plain_sampled": round(G / best / (1e3 / ms_tok_sampled), 3)}
            out["sampled"] = rec
        emit(**out)
        st.close(), mt.close()
m.close()
be.close()
