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

Positional: model, batches ("2,4,8"), tokens_per_seq values ("2,4"), tokens, start, reps. Flags:
  --max-seq S    context length of the plans (default 512 for llama2-7b, else 2048)
  --option V     ZGML_HIP_OPT_SMALL_M_MATVEC at compile (default 1: the row kernel up to its measured bound, M <= 6)"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, llama  # noqa: E402


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
table = []


def emit(**kw):
    print(json.dumps({"model": name, "positions": [start, start + tokens], "option": option, **kw}), flush=True)


def timed(call):
    call()  # warm-up
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    assert not be.last_error(), be.last_error()
    return times, out


for B in batches:
    first = [(911 * b + 17) % cfg.vocab_size for b in range(B)]
    bs = llama.BatchSession(m, fns, B, small_m_matvec=option)
    bs.resident_setup(be)
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
        for form, drafts in forms.items():
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
m.close()
be.close()
