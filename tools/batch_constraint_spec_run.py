"""What speculation under token automata gives a BATCH (zgml_hip_resident_decode_batch_speculative_constrained, include/zgml_hip.h)
over the one-token-per-step-and-sequence constrained batched loop. The TEMPLATE automaton of tools/constraint_spec_run.py — free
states that allow three of four hashed classes, then a literal run of forced tokens, in a cycle — at three forced-token shares
(0 %, about 30 %, about 60 % of the emitted tokens), attached to EVERY sequence; its sampling parameters, sequence b on stream b.
Per (B, Ts, share), in one process, alternating inside every repetition, one untimed run of each first (graph capture):
    spec              the new call on the B x Ts plan, n-gram lookup drafts (a forced token needs none)
    sampled           zgml_hip_resident_decode_batch_sampled on the one-column plan of the same B with the SAME automata from the
                      same states
One JSON line per cell with every repetition's figure; then a table: tokens per step and sequence, ms per step, tok/s of all
sequences of both, and the ratio spec / sampled (best of `reps` each). Everything printed is also APPENDED to
profiles/r24_batch_constraint_spec.txt (--profile names another file, --profile - none), behind a line with the command.

    timeout -k 10 500 python tools/batch_constraint_spec_run.py smollm-135m 2,4,8 4,8 256 3 --explain

    argv: preset [batches = 2,4,8] [tokens_per_seq values = 4,8] [tokens = 128] [reps = 3] [--base] [--explain] [--profile FILE]

The two calls run DIFFERENT plans, so their streams need not be equal (a KV column stored as a later row of a
step is not bit-equal to the same column stored one per step, a pick may turn on the last bit of the logits, and a sampled stream
that took another token once goes another way from there). Every line carries `first_diff`, per sequence the first token index at
which the two streams differ (null: equal). --explain: for every cell with a difference the B x Ts plan is also driven from the
HOST in lock-step (tests/batch_spec_constraint_model.py: one BatchSession.step per verify step, all rows downloaded, every row
picked on the CPU by zgml_amd/csrc/sample.h) and the line carries `replay` — whether that replay gives the device call's tokens,
steps and states, i.e. whether the call's stream is what ITS plan's logits give —, and at the first differing index of the first
differing sequence the two tokens, their ranks among the row's constrained candidates and their logits in the replayed row.

--base: only the calls that the build before this one has too, for runs of two builds in fresh processes (ZGML_HIP_LIB names the
other build's library): per (B, Ts) the constrained one-column zgml_hip_resident_decode_batch_sampled step at the 30 % share and
the UNCONSTRAINED zgml_hip_resident_decode_batch_speculative_sampled step (n-gram drafts), every repetition's µs per step, and a
checksum of the tokens of each.

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it, and attaching the automata lies outside it. Checked as well: every constrained token
is allowed in the state it was picked in, the device's final state is the one the tokens lead to; the measured forced share is
reported."""
import json
import sys
import time
import zlib
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
from zgml_amd import Backend, capi, llama  # noqa: E402

args = [a for a in sys.argv[1:] if a not in ("--base", "--explain")]
base_only, explain_diffs = "--base" in sys.argv[1:], "--explain" in sys.argv[1:]
ROOT = Path(__file__).resolve().parent.parent
profile = str(ROOT / "profiles" / "r24_batch_constraint_spec.txt")
if "--profile" in args:
    profile = args[args.index("--profile") + 1]
    del args[args.index("--profile"):args.index("--profile") + 2]


def say(text=""):
    """to stdout and, appended, to the profile"""
    print(text, flush=True)
    if profile != "-":
        with open(profile, "a") as f:
            f.write(text + "\n")


say("\n== python tools/batch_constraint_spec_run.py " + " ".join(sys.argv[1:]))
arg = lambda i, default, kind: kind(args[i]) if len(args) > i else default  # noqa: E731
ints = lambda text: [int(x) for x in text.split(",")]  # noqa: E731
name, batches, widths, n, reps = arg(0, "smollm-135m", str), arg(1, [2, 4, 8], ints), arg(2, [4, 8], ints), arg(3, 128, int), arg(4, 3, int)

be = Backend(0)
cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
assert n + max(widths) <= cfg.max_seq_len
V = cfg.vocab_size
m = llama.Model(cfg, llama.Q4_0, threads=16)
fns = llama.hip_backend_fns(be)
print("model built", file=sys.stderr, flush=True)


def template(free, run, seed):
    """`free` free states (classes 0..2 of 4 hashed ones allowed) then `run` literal states, in a cycle -> (class_of, next)"""
    rng = np.random.default_rng(seed)
    i = np.arange(V, dtype=np.uint64)
    cls = (((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(4)).astype(np.uint16)
    lits = rng.choice(V, run, replace=False)
    cls[lits] = 4 + np.arange(run, dtype=np.uint16)
    nxt = np.full((free + run, 4 + run), 0xFFFF, np.uint16)
    for st in range(free + run):
        if st < free:
            nxt[st, :3] = (st + 1) % (free + run)
        else:
            nxt[st, 4 + st - free] = (st + 1) % (free + run)
    return cls, nxt


shares = {"30": (7, 3)} if base_only else {"0": (1, 0), "30": (7, 3), "60": (4, 6)}
tables = {k: template(f, r, 7 + r) for k, (f, r) in shares.items()}
cons = {k: be.constraint_create(*t) for k, t in tables.items()}


def attach(s, B, k):
    for b in range(B):
        s.set_constraint(cons[k] if k is not None else None, 0, seq=b)


def walk(k, toks, state):
    """-> the forced tokens among toks; every token is allowed where it was picked and `state` is where they lead"""
    cls, nxt = tables[k]
    st, forced = 0, 0
    for t in toks:
        forced += int(cls[t]) >= 4
        st = int(nxt[st, cls[t]])
        assert st != 0xFFFF, "a token that its state forbids"
    assert st == state, "the device's state is not the walk's"
    return forced


def timed(calls):
    """the calls alternate repetition by repetition -> per call (seconds of every timed repetition, the result)"""
    secs, outs = [[] for _ in calls], [None for _ in calls]
    for rep in range(reps + 1):  # (rep 0: untimed)
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            out = c()
            dt = time.perf_counter() - t0
            assert outs[i] is None or outs[i] == out, "a repetition produced another result"
            outs[i] = out
            if rep:
                secs[i].append(dt)
    assert not be.last_error(), be.last_error()
    return list(zip(secs, outs))


def first_diffs(a, b):
    """per sequence the first index at which the streams differ, None: equal"""
    return [next((i for i, (x, y) in enumerate(zip(ra, rb)) if x != y), None) for ra, rb in zip(a, b)]


def explain(B, Ts, k, firsts, sps, o_x, o_s, diffs):
    """the B x Ts plan driven from the host in lock-step: is the device call's stream what its own plan's logits give? And what
    the replayed row at the first difference says of the two tokens"""
    from tests import batch_spec_constraint_model as BCM
    from tests.test_constraint_host import Dfa, c_constraint_candidates
    host = llama.BatchSession(m, fns, B, tokens_per_seq=Ts)
    dfa = Dfa(*tables[k])
    b = next(q for q, d in enumerate(diffs) if d is not None)
    i, keep, seqs = diffs[b], {}, []

    def step(toks, pos):
        logits = host.step(toks, pos)[1]
        j = i - pos[b]  # (token index i is picked from the row at position i: the last step that computes it is the one that emits it)
        if 0 <= j < Ts:
            keep["row"] = np.array(logits[b * Ts + j], np.float32)
        return logits

    toks, produced, stats, _, states = BCM.lockstep(step, Ts, [BCM.Request(firsts[q], 0, n, sps[q], dfa=dfa, state=0) for q in range(B)], seqs_out=seqs)
    host.close()
    same = toks.tolist() == o_x[0] and [st["steps"] for st in stats] == o_x[1] and states == o_x[2]
    state = seqs[b].seen[i][0]
    cands = [int(t) for t in c_constraint_candidates(keep["row"], sps[b], None, dfa, state)]
    t_x, t_s = o_x[0][b][i], o_s[0][b][i]
    rank = lambda t: cands.index(t) if t in cands else None  # noqa: E731
    return {"replay_equals_device_call": same, "sequence": b, "index": i, "state": state, "spec_token": t_x, "sampled_token": t_s,
            "rank_in_replayed_row": {"spec": rank(t_x), "sampled": rank(t_s)}, "candidates": len(cands),
            "logit_in_replayed_row": {"spec": float(keep["row"][t_x]), "sampled": float(keep["row"][t_s])}}


table = []
for B in batches:
    firsts, starts = [(911 * b + 17) % V for b in range(B)], [0] * B
    sps = [capi.SamplingC.of(temperature=0.8, top_k=40, top_p=0.95, seed=1, stream=b) for b in range(B)]
    s1 = llama.BatchSession(m, fns, B)
    s1.resident_setup(be)
    for Ts in widths:
        sT = llama.BatchSession(m, fns, B, tokens_per_seq=Ts)
        sT.resident_setup(be)

        def sampled(k):
            attach(s1, B, k)
            toks, produced = s1.resident_decode_batch_sampled(firsts, starts, n, sps)
            assert (produced == n).all()
            return toks.tolist(), [n] * B, [s1.constraint_state(seq=b) for b in range(B)]

        def spec(k):
            attach(sT, B, k)
            toks, produced, stats = sT.resident_decode_batch_speculative_constrained(firsts, starts, n, sps)
            assert (produced == n).all()
            return toks.tolist(), [st["steps"] for st in stats], [sT.constraint_state(seq=b) for b in range(B)]

        def plain_spec():
            attach(sT, B, None)
            toks, produced, stats = sT.resident_decode_batch_speculative_sampled(firsts, starts, n, sps)
            assert (produced == n).all()
            return toks.tolist(), [st["steps"] for st in stats], None

        for k in shares:
            if base_only:
                (t_s, o_s), (t_p, o_p) = timed([lambda: sampled(k), plain_spec])
                crc = lambda o: zlib.crc32(np.asarray(o[0], np.int64).tobytes())  # noqa: E731
                say(json.dumps({"model": name, "base": True, "B": B, "Ts": Ts, "tokens": n, "reps": reps,
                                  "batch_sampled_constrained_step_us": [round(1e6 * t / n, 2) for t in t_s], "batch_sampled_constrained_tokens_crc": crc(o_s),
                                  "batch_spec_sampled_step_us": [round(1e6 * t / max(o_p[1]), 2) for t in t_p], "batch_spec_sampled_steps": max(o_p[1]),
                                "batch_spec_sampled_tokens_crc": crc(o_p)}))
                continue
            (t_x, o_x), (t_s, o_s) = timed([lambda: spec(k), lambda: sampled(k)])
            share = [round(sum(walk(k, o[0][b], o[2][b]) for b in range(B)) / (B * n), 3) for o in (o_x, o_s)]
            steps = max(o_x[1])  # steps the call ran, for its slowest sequence
            per_step = sum(n / st for st in o_x[1]) / B
            tok_s = [[round(B * n / t, 1) for t in ts] for ts in (t_x, t_s)]
            ms = [round(1e3 * min(t_x) / steps, 4), round(1e3 * min(t_s) / n, 4)]
            ratio = round(max(tok_s[0]) / max(tok_s[1]), 3)
            diffs = first_diffs(o_x[0], o_s[0])
            why = None
            if explain_diffs and any(d is not None for d in diffs):
                try:
                    why = explain(B, Ts, k, firsts, sps, o_x, o_s, diffs)
                except Exception as e:  # (the figures of the cell stand without it)
                    why = {"error": repr(e)}
            say(json.dumps({"model": name, "B": B, "Ts": Ts, "share": k, "tokens": n, "reps": reps, "forced_share": {"spec": share[0], "sampled": share[1]},
                              "steps": o_x[1], "tokens_per_step_and_seq": round(per_step, 3), "ms_per_step": {"spec": ms[0], "sampled": ms[1]},
                              "step_ratio": round(ms[0] / ms[1], 3), "tok_s": {"spec": tok_s[0], "sampled": tok_s[1]}, "spec_over_sampled": ratio,
                              "same_tokens": o_x[0] == o_s[0], "first_diff": diffs, "replay": why}))
            table.append((B, Ts, k, share[0], per_step, ms[0], ms[1], max(tok_s[0]), max(tok_s[1]), ratio))
        attach(sT, B, None)
        sT.close()
    attach(s1, B, None)
    s1.close()

if table:
    say(f"\n{name}: {n} tokens per sequence from position 0, n-gram drafts, best of {reps}; sampled = the one-column constrained batched loop")
    say(f"{'B':>3} {'Ts':>3} {'share':>6} {'forced':>7} {'tok/step/seq':>13} {'spec ms':>9} {'sampled ms':>11} {'spec tok/s':>11} {'sampled tok/s':>14} {'ratio':>7}")
    for B, Ts, k, sh, per, ms_x, ms_s, tx, ts, ratio in table:
        say(f"{B:>3} {Ts:>3} {k:>6} {sh:>7.3f} {per:>13.3f} {ms_x:>9.4f} {ms_s:>11.4f} {tx:>11.1f} {ts:>14.1f} {ratio:>7.3f}")
for c in cons.values():
    be.constraint_free(c)
m.close()
be.close()
