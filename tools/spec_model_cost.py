"""What a verify step with a draft model costs (zgml_hip_resident_decode_speculative_model), per target model and T:

  t_step     the pair's call over `tokens` tokens from position 0, per verify step that ran (idle ones included: the target's
             call_count says how many)
  t_ngram    the step of zgml_hip_resident_decode_speculative on the SAME T-plan (provided mode without drafts, pads alone: the
             chain of the n-gram step, which is the pair's chain without the T draft executions), per step that ran
  t_token    the plain resident loop (zgml_hip_resident_decode) on the target's token_len = 1 plan over the same positions
  draft      t_step - t_ngram: the part of a step that is the T draft executions
  break-even t_step / t_token: the tokens a step must emit on average for the pair to match the plain loop

    timeout -k 10 300 python tools/spec_model_cost.py smollm-135m 2 && timeout -k 10 900 python tools/spec_model_cost.py llama2-7b 1,2

--batch 2,4,8: the batched pair instead (zgml_hip_resident_decode_batch_speculative_model), per B and T — every sequence the same
request, `tokens` tokens from position 0: t_step of the pair, t_ngram of zgml_hip_resident_decode_batch_speculative on the same
B x T plan (provided mode without drafts), t_token the step of zgml_hip_resident_decode_batch at the same B (one token per
sequence), break-even t_step / t_token: the tokens PER SEQUENCE a step must emit on average to match the batched plain loop.

    timeout -k 10 600 python tools/spec_model_cost.py smollm-135m 2 2,4 --batch 2,4,8

Positional: model, draft layer counts ("1,2": drafts of the target's dimensions with that many layers), T values ("2,4,5"), tokens,
reps. --max-seq S (default 512). Synthetic Q4_0 weights: the acceptance printed is that of two unrelated synthetic models and says
nothing about trained ones — only the times do. Each run is a blocking call that ends with the tokens on the host; the clock is the
host's around it, best of `reps` after one warm-up (which also captures the graph); pair, n-gram and plain calls alternate."""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402

args = sys.argv[1:]
max_seq = 512
if "--max-seq" in args:
    i = args.index("--max-seq")
    max_seq = int(args[i + 1])
    del args[i:i + 2]
batches = []
if "--batch" in args:
    i = args.index("--batch")
    batches = [int(x) for x in args[i + 1].split(",")]
    del args[i:i + 2]
name = args[0] if len(args) > 0 else "smollm-135m"
draft_layers = [int(x) for x in args[1].split(",")] if len(args) > 1 else [2]
widths = [int(x) for x in args[2].split(",")] if len(args) > 2 else [2, 4, 5]
tokens = int(args[3]) if len(args) > 3 else 128
reps = int(args[4]) if len(args) > 4 else 3
FIRST = 17

be = Backend(0)
fns = llama.hip_backend_fns(be)
cfg = llama.preset(name, max_seq)
assert tokens + max(widths) <= cfg.max_seq_len, "positions beyond --max-seq"
target = llama.Model(cfg, llama.Q4_0, threads=16)


def session(model, small_m=None):
    if small_m is not None:
        be.set_option(capi.OPT_SMALL_M_MATVEC, small_m)
    try:
        s = llama.Session(model, fns)
    finally:
        be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    s.resident_setup(be)
    return s


def steps_of(handle, call):
    before = int(be.getRuntimeProfile(handle).call_count)
    out = call()
    return int(be.getRuntimeProfile(handle).call_count) - before, out


def timed(calls):
    """best-of-reps seconds of every call, alternating repetition by repetition after one warm-up each"""
    for c in calls:
        c()
    best = [float("inf")] * len(calls)
    for _ in range(reps):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            c()
            best[i] = min(best[i], time.perf_counter() - t0)
    assert not be.last_error(), be.last_error()
    return best


def batched():
    """the --batch table: per B a one-column batched plain loop and one batched draft per layer count, per T the B x T target"""
    table = []
    for B in batches:
        firsts, starts = [FIRST + b for b in range(B)], [0] * B
        pm = llama.BatchModel(None, B, like=target)
        ps = llama.BatchSession(pm, fns, B)
        ps.resident_setup(be)
        bdrafts = {}
        for L in draft_layers:
            dcfg = llama.preset(name, max_seq)
            dcfg.n_layers = L
            dm = llama.BatchModel(dcfg, B, llama.Q4_0, threads=16)
            ds = llama.BatchSession(dm, fns, B)
            ds.resident_setup(be)
            bdrafts[L] = (ds, dm)
        for T in widths:
            tm = llama.BatchModel(None, B, like=target, tokens_per_seq=T)
            ts = llama.BatchSession(tm, fns, B)
            ts.resident_setup(be)
            print(f"# B {B} T {T}: sessions built", file=sys.stderr, flush=True)
            ngram = lambda: ts.resident_decode_batch_speculative(firsts, starts, tokens, drafts=[[]] * B)
            n_steps, _ = steps_of(ts.handle, ngram)
            for L, (ds, _) in bdrafts.items():
                pair = lambda: ts.resident_decode_batch_speculative_model(ds, firsts, starts, tokens)
                steps, (_, _, stats) = steps_of(ts.handle, pair)
                t_pair, t_ngram, t_plain = timed([pair, ngram, lambda: ps.resident_decode_batch(firsts, starts, tokens)])
                row = dict(model=name, B=B, T=T, draft_layers=L, tokens=tokens, steps_run=steps, stats=stats[0],
                           launches_target=be.planText(ts.handle).count("\n") + 4, launches_draft_per_step=T * (be.planText(ds.handle).count("\n") + 3),
                           t_step_us=round(1e6 * t_pair / steps, 2), t_ngram_step_us=round(1e6 * t_ngram / n_steps, 2), t_token_us=round(1e6 * t_plain / tokens, 2))
                row["draft_part_us"] = round(row["t_step_us"] - row["t_ngram_step_us"], 2)
                row["break_even_tokens_per_step_per_seq"] = round(row["t_step_us"] / row["t_token_us"], 3)
                row["break_even_ngram"] = round(row["t_ngram_step_us"] / row["t_token_us"], 3)
                print(json.dumps(row), flush=True)
                table.append(row)
            ts.close(), tm.close()
        for ds, dm in bdrafts.values():
            ds.close(), dm.close()
        ps.close(), pm.close()
    print(f"\n{name}, max_seq {max_seq}, batched: {tokens} tokens per sequence from position 0, best of {reps}; synthetic Q4_0 weights (acceptance on trained weights: not measured)")
    print(f"{'B':>2} {'T':>2} {'draft L':>7} {'t_step us':>10} {'n-gram step us':>15} {'t_token us':>11} {'draft part us':>14} {'break-even':>11} {'(n-gram)':>9}")
    for r in table:
        print(f"{r['B']:>2} {r['T']:>2} {r['draft_layers']:>7} {r['t_step_us']:>10.1f} {r['t_ngram_step_us']:>15.1f} {r['t_token_us']:>11.1f} {r['draft_part_us']:>14.1f} "
              f"{r['break_even_tokens_per_step_per_seq']:>11.3f} {r['break_even_ngram']:>9.3f}")


if batches:
    batched()
    target.close(), be.close()
    sys.exit(0)

plain = session(target)
drafts = {}
for L in draft_layers:
    dcfg = llama.preset(name, max_seq)
    dcfg.n_layers = L
    dm = llama.Model(dcfg, llama.Q4_0, threads=16)
    drafts[L] = (session(dm), dm)

table = []
for T in widths:
    tm = llama.Model(None, token_len=T, like=target)
    ts = session(tm, small_m=1)
    n_steps, (_, st_ngram) = steps_of(ts.handle, lambda: ts.resident_decode_speculative(FIRST, 0, tokens, drafts=[]))
    assert n_steps >= st_ngram["steps"] > 0
    for L, (ds, _) in drafts.items():
        steps, (_, stats) = steps_of(ts.handle, lambda: ts.resident_decode_speculative_model(ds, FIRST, 0, tokens))
        t_pair, t_ngram, t_plain = timed([lambda: ts.resident_decode_speculative_model(ds, FIRST, 0, tokens),
                                          lambda: ts.resident_decode_speculative(FIRST, 0, tokens, drafts=[]),
                                          lambda: plain.resident_decode(FIRST, 0, tokens)])
        row = dict(model=name, T=T, draft_layers=L, tokens=tokens, steps_run=steps, stats=stats,
                   launches_target=be.planText(ts.handle).count("\n") + 4, launches_draft_per_step=T * (be.planText(ds.handle).count("\n") + 3),
                   t_step_us=round(1e6 * t_pair / steps, 2), t_ngram_step_us=round(1e6 * t_ngram / n_steps, 2), t_token_us=round(1e6 * t_plain / tokens, 2))
        row["draft_part_us"] = round(row["t_step_us"] - row["t_ngram_step_us"], 2)
        row["draft_share"] = round(row["draft_part_us"] / row["t_step_us"], 3)
        row["break_even_tokens_per_step"] = round(row["t_step_us"] / row["t_token_us"], 3)
        row["break_even_ngram"] = round(row["t_ngram_step_us"] / row["t_token_us"], 3)
        print(json.dumps(row), flush=True)
        table.append(row)
    ts.close(), tm.close()

print(f"\n{name}, max_seq {max_seq}: {tokens} tokens from position 0, best of {reps}; synthetic Q4_0 weights (acceptance on trained weights: not measured)")
print(f"{'T':>2} {'draft L':>7} {'t_step us':>10} {'n-gram step us':>15} {'t_token us':>11} {'draft part us':>14} {'share':>6} {'break-even':>11} {'(n-gram)':>9}")
for r in table:
    print(f"{r['T']:>2} {r['draft_layers']:>7} {r['t_step_us']:>10.1f} {r['t_ngram_step_us']:>15.1f} {r['t_token_us']:>11.1f} {r['draft_part_us']:>14.1f} "
          f"{r['draft_share']:>6.3f} {r['break_even_tokens_per_step']:>11.3f} {r['break_even_ngram']:>9.3f}")
for ds, dm in drafts.values():
    ds.close(), dm.close()
plain.close(), target.close(), be.close()
