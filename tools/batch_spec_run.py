"""Speculative decode under batching (zgml_hip_resident_decode_batch_speculative) of one model: for every (B, Ts) the B x Ts plan's
verify loop with provided drafts that are all right (the ceiling: Ts tokens per sequence and step) and all wrong (the price of a
step: one token per sequence and step), next to zgml_hip_resident_decode_batch on the one-column plan of the same B over the same
positions (that plan is op for op the one the builder made before it took tokens_per_seq, and the loop over it is unchanged). One
JSON line per run group with every repetition's figure, then a table: tok/s of all sequences, ms per step, and the break-even
accepted tokens per step and sequence, t_step(B, Ts) / t_step(B, 1).

    timeout -k 10 400 python tools/batch_spec_run.py smollm-135m && timeout -k 10 900 python tools/batch_spec_run.py llama2-7b

(llama2-7b: all 32 layers, synthetic Q4_0 GGUF-valued weights, max_seq 512.) Every sequence produces `tokens` tokens from position
`start`: positions [start, start + tokens), whatever the number of steps that takes. Each run is a blocking call that ends with the
tokens on the host; the clock is the host's around it, `reps` timed runs after one warm-up (which also captures the graph). The
"right" drafts are the tokens of a first run of the same plan with n-gram drafts; where the plan's rows differ between step
alignments (near-ties of the synthetic LM head) some are rejected, so the line carries the tokens per step that were really emitted.

With --sampled (say --sampled 0.8,40,0.95,1) every run group is followed by its sampled twin on the SAME program, greedy and
sampled calls alternating repetition by repetition: zgml_hip_resident_decode_batch_sampled beside the one-column greedy loop,
zgml_hip_resident_decode_batch_speculative_sampled beside the greedy verify loop (sequence b samples with stream + b). The sampled
drafts are the tokens of a first sampled run of the same plan with n-gram drafts. The table then carries, per (B, Ts, drafts), the
sampled step next to the greedy one, their difference, and the sampled break-even against the one-column SAMPLED loop.

Positional: model, batches ("2,4,8"), tokens_per_seq values ("2,4"), tokens, start, reps. Flags:
  --max-seq S    context length of the plans (default 512 for llama2-7b, else 2048)
  --option V     ZGML_HIP_OPT_SMALL_M_MATVEC at compile (default 1: the row kernel up to its measured bound, M <= 6)
  --sampled temperature,top_k,top_p,stream   also the sampled calls (seed 1234), alternating with the greedy ones"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402


def take_flag(args, name):
    if name not in args:
        return None
    i = args.index(name)
    value = args[i + 1]
    del args[i:i + 2]
    return value


args = sys.argv[1:]
max_seq = int(take_flag(args, "--max-seq") or 0)
option = int(take_flag(args, "--option") or 1)
sampled = take_flag(args, "--sampled")
name = args[0] if len(args) > 0 else "smollm-135m"
batches = [int(b) for b in args[1].split(",")] if len(args) > 1 else [2, 4, 8]
widths = [int(t) for t in args[2].split(",")] if len(args) > 2 else [2, 4]
tokens = int(args[3]) if len(args) > 3 else 256
start = int(args[4]) if len(args) > 4 else 4
reps = int(args[5]) if len(args) > 5 else 3

be = Backend(0)
cfg = llama.preset(name, max_seq or (512 if name == "llama2-7b" else 2048))
assert start + tokens + max(widths) <= cfg.max_seq_len, "positions beyond --max-seq"
m = llama.Model(cfg, llama.Q4_0, threads=16)
fns = llama.hip_backend_fns(be)
table, table_s = [], []


def samplings(B):
    """one parameter set per sequence: the flag's, stream + b"""
    t, k, p, stream = sampled.split(",")
    return [capi.SamplingC.of(float(t), int(k), float(p), seed=1234, stream=int(stream) + b) for b in range(B)]


def emit(**kw):
    print(json.dumps({"model": name, "positions": [start, start + tokens], "option": option, **kw}), flush=True)


def timed(call, twin=None):
    """-> (times, last result) of `call`; with `twin` — the sampled call on the same program — the two alternate repetition by
    repetition and the twin's (times, last result) follow"""
    calls = [call] + ([twin] if twin else [])
    for c in calls:
        c()  # warm-up
    times, out = [[] for _ in calls], [None for _ in calls]
    for _ in range(reps):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            out[i] = c()
            times[i].append(time.perf_counter() - t0)
    assert not be.last_error(), be.last_error()
    return (times[0], out[0], times[1], out[1]) if twin else (times[0], out[0])


for B in batches:
    first = [(911 * b + 17) % cfg.vocab_size for b in range(B)]
    bs = llama.BatchSession(m, fns, B, small_m_matvec=option)
    bs.resident_setup(be)
    base_step_s = None
    if sampled:
        sps = samplings(B)
        times, toks, times_s, (toks_s, made) = timed(lambda: bs.resident_decode_batch(first, [start] * B, tokens),
                                                     lambda: bs.resident_decode_batch_sampled(first, [start] * B, tokens, sps))
        assert (toks_s >= 0).all() and (made == tokens).all()
        base_step_s = min(times_s) / tokens
        emit(path="batch_sampled", B=B, Ts=1, sampling=sampled, launches=be.planText(bs.handle).count("\n") + 3,
             ms_per_step=[round(1e3 * t / tokens, 4) for t in times_s], tok_s=[round(B * tokens / t, 1) for t in times_s])
        table_s.append((B, 1, "batch_sampled", B * tokens / min(times_s), 1e3 * min(times) / tokens, 1e3 * base_step_s, 1.0, None))
    else:
        times, toks = timed(lambda: bs.resident_decode_batch(first, [start] * B, tokens))
    assert toks.shape == (B, tokens) and (toks >= 0).all()
    base_step = min(times) / tokens
    emit(path="batch", B=B, Ts=1, launches=be.planText(bs.handle).count("\n") + 3, ms_per_step=[round(1e3 * t / tokens, 4) for t in times],
         tok_s=[round(B * tokens / t, 1) for t in times])
    table.append((B, 1, "decode_batch", B * tokens / min(times), 1e3 * base_step, 1.0, None))
    bs.close()
    for Ts in widths:
        s = llama.BatchSession(m, fns, B, small_m_matvec=option, tokens_per_seq=Ts)
        s.resident_setup(be)
        text = be.planText(s.handle)
        stream, _ = s.resident_decode_batch_speculative(first, [start] * B, tokens)  # n-gram drafts: the plan's own greedy tokens
        assert not be.last_error(), be.last_error()
        pad = [[int(t) for t in row] + [int(row[-1])] * Ts for row in stream]
        forms = {"right": pad, "wrong": [[(t + 1) % cfg.vocab_size for t in row] for row in pad]}
        if sampled:  # the sampled stream of THIS plan, from a sampled run with n-gram drafts
            stream_s = s.resident_decode_batch_speculative_sampled(first, [start] * B, tokens, sps)[0]
            assert not be.last_error(), be.last_error()
            pad_s = [[int(t) for t in row] + [int(row[-1])] * Ts for row in stream_s]
            forms_s = {"right": pad_s, "wrong": [[(t + 1) % cfg.vocab_size for t in row] for row in pad_s]}
        for form, drafts in forms.items():
            if sampled:
                times, (toks, stats), times_s, (toks_s, made, stats_s) = timed(
                    lambda: s.resident_decode_batch_speculative(first, [start] * B, tokens, drafts=drafts),
                    lambda: s.resident_decode_batch_speculative_sampled(first, [start] * B, tokens, sps, drafts=forms_s[form]))
                assert (made == tokens).all()
                steps_s = max(st["steps"] for st in stats_s)
                per_step_s = sum(tokens / st["steps"] for st in stats_s) / B
                step_ms_s = 1e3 * min(times_s) / steps_s
                emit(path="batch_spec_sampled", B=B, Ts=Ts, drafts=form, sampling=sampled, launches=text.count("\n") + 5, steps=[st["steps"] for st in stats_s],
                     tokens_per_step_and_seq=round(per_step_s, 3), same_tokens_as_ngram_run=toks_s.tolist() == stream_s.tolist(),
                     ms_per_step=[round(1e3 * t / steps_s, 4) for t in times_s], tok_s=[round(B * tokens / t, 1) for t in times_s])
                greedy_ms = 1e3 * min(times) / max(st["steps"] for st in stats)
                table_s.append((B, Ts, form, B * tokens / min(times_s), greedy_ms, step_ms_s, step_ms_s / (1e3 * base_step_s), per_step_s))
            else:
                times, (toks, stats) = timed(lambda: s.resident_decode_batch_speculative(first, [start] * B, tokens, drafts=drafts))
            assert toks.tolist() == stream.tolist() or form == "right", "the drafts changed the tokens"
            steps = max(st["steps"] for st in stats)  # steps the call ran for its slowest sequence
            per_step = sum(tokens / st["steps"] for st in stats) / B
            emit(path="batch_spec", B=B, Ts=Ts, drafts=form, launches=text.count("\n") + 4, attention_launches=text.count("kind 10 "),
                 steps=[st["steps"] for st in stats], tokens_per_step_and_seq=round(per_step, 3), same_tokens_as_ngram_run=toks.tolist() == stream.tolist(),
                 ms_per_step=[round(1e3 * t / steps, 4) for t in times], tok_s=[round(B * tokens / t, 1) for t in times])
            step_ms = 1e3 * min(times) / steps
            table.append((B, Ts, form, B * tokens / min(times), step_ms, step_ms / (1e3 * base_step), per_step))
        s.close()

print(f"\n{name}: {tokens} tokens per sequence from position {start}, best of {reps}; break-even = ms/step over the one-column loop's at the same B")
print(f"{'B':>3} {'Ts':>3} {'drafts':>13} {'tok/s':>9} {'ms/step':>9} {'break-even':>11} {'tok/step/seq':>13}")
for B, Ts, form, tps, ms, be_even, per in table:
    print(f"{B:>3} {Ts:>3} {form:>13} {tps:>9.1f} {ms:>9.4f} {be_even:>11.3f} {'' if per is None else f'{per:>13.3f}'}")
if sampled:
    print(f"\n{name}, sampled ({sampled}; seed 1234, stream + b): the sampled step beside the greedy step of the same program, alternating; "
          "break-even = sampled ms/step over the one-column SAMPLED loop's at the same B")
    print(f"{'B':>3} {'Ts':>3} {'drafts':>13} {'tok/s':>9} {'greedy ms':>10} {'sampled ms':>11} {'diff us':>8} {'break-even':>11} {'tok/step/seq':>13}")
    for B, Ts, form, tps, g_ms, s_ms, be_even, per in table_s:
        print(f"{B:>3} {Ts:>3} {form:>13} {tps:>9.1f} {g_ms:>10.4f} {s_ms:>11.4f} {1e3 * (s_ms - g_ms):>8.1f} {be_even:>11.3f} {'' if per is None else f'{per:>13.3f}'}")
m.close()
be.close()
