"""What speculation under a token automaton (zgml_hip_resident_decode_speculative_constrained, include/zgml_hip.h) gives over the
one-token-per-launch constrained loop, and that an unconstrained sampled speculative call costs what it did. A TEMPLATE automaton
— free states that allow three of four hashed classes, then a literal run of forced tokens, in a cycle — at three forced-token
shares (0 %, about 30 %, about 60 % of the emitted tokens); per share, in one process, alternating inside every repetition, one
untimed run of each first (graph capture):
    spec_T            the new call on a token_len = T plan, n-gram lookup drafts (a forced token needs none)
    sampled           zgml_hip_resident_decode_sampled on the token_len = 1 plan with the SAME automaton from the same state
and, with nothing attached,
    plain_spec        zgml_hip_resident_decode_speculative_sampled on the T plan, this build
    parent_spec       the same call of ANOTHER build of the library — the parent commit's, given as argv[5] — on a context and a
                      program of its own over the same weights
One JSON line: tokens per step and tok/s of every variant (every repetition kept), µs per verify step of the two unconstrained
ones with their spread, and `break_even_share`, the forced share at which spec_T's tok/s crosses sampled's (linear between the
measured shares; null when it never does, 0 when it is ahead everywhere).

    timeout -k 10 600 python tools/constraint_spec_run.py smollm-135m 4 192 5 /path/to/parent/libzgml_hip.so

    argv: preset [T = 4] [tokens = 192] [reps = 5] [parent library = none] [parent_first = 0]

(parent_first = 1 creates the parent build's context and program before this build's: two contexts of one process differ by a
few µs per step whichever build they run, and swapping them tells that apart from a difference between the builds.)

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it, and attaching the automaton lies outside it. Checked as well: every constrained
token is allowed in the state it was picked in, the device's final state is the one the tokens lead to, the measured forced share
is reported, and plain_spec and parent_spec give the same tokens and statistics."""
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
T, n, reps, parent, parent_first = arg(2, 4, int), arg(3, 192, int), arg(4, 5, int), arg(5, "", str), arg(6, 0, int)

libs = {"this": capi.load_hip()}
if parent:
    libs["parent"] = C.CDLL(parent)
    capi._bind_hip(libs["parent"])


def use(which):  # (the Python wrappers ask capi.load_hip() at every call)
    capi._hip_lib = libs[which]


cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
assert n + T <= cfg.max_seq_len
V, first = cfg.vocab_size, 1
mT, m1 = llama.Model(cfg, llama.Q4_0, threads=16, token_len=T), llama.Model(cfg, llama.Q4_0, threads=16)
print("models built", file=sys.stderr, flush=True)
side = {}
for which in (reversed(list(libs)) if parent_first else libs):
    use(which)
    be = Backend(0)
    sT = llama.Session(mT, llama.hip_backend_fns(be))
    sT.resident_setup(be)
    side[which] = (be, sT)
use("this")
be, sT = side["this"]
s1 = llama.Session(m1, llama.hip_backend_fns(be))
s1.resident_setup(be)


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


shares = {"0": (1, 0), "30": (7, 3), "60": (4, 6)}
tables = {k: template(f, r, 7 + r) for k, (f, r) in shares.items()}
cons = {k: be.constraint_create(*t) for k, t in tables.items()}
S = capi.SamplingC.of
sp = S(temperature=0.8, top_k=40, top_p=0.95, seed=1)

# variant -> one call: (tokens, steps)
def spec(k):
    sT.set_constraint(cons[k], 0)
    toks, produced, stats = sT.resident_decode_speculative_constrained(first, 0, n, sp)
    assert produced == n
    return toks.tolist(), stats["steps"], sT.constraint_state()


def sampled(k):
    s1.set_constraint(cons[k], 0)
    toks, produced = s1.resident_decode_sampled(first, 0, n, sp)
    assert produced == n
    return toks.tolist(), n, s1.constraint_state()


def plain_spec(which):
    def run(_):
        use(which)
        if which == "this":
            sT.set_constraint(None)
        toks, produced, stats = side[which][1].resident_decode_speculative_sampled(first, 0, n, sp)
        use("this")
        return toks.tolist(), (stats["steps"], stats["drafted"], stats["accepted"]), -1
    return run


variants = {}
for k in shares:
    variants["spec_T_" + k] = (spec, k)
    variants["sampled_" + k] = (sampled, k)
variants["plain_spec"] = (plain_spec("this"), None)
if parent:
    variants["parent_spec"] = (plain_spec("parent"), None)

secs, outs = {v: [] for v in variants}, {}
for rep in range(reps + 1):  # (rep 0: untimed)
    print("repetition", rep, file=sys.stderr, flush=True)
    for v, (fn, k) in variants.items():
        t0 = time.perf_counter()
        out = fn(k)
        dt = time.perf_counter() - t0
        assert outs.setdefault(v, out) == out, v + ": a repetition produced another result"
        if rep:
            secs[v].append(dt)
for b, _ in side.values():
    assert not b.last_error(), b.last_error()
forced_share = {}
for v, (fn, k) in variants.items():  # every constrained token is allowed where it was picked; the state is the walk's
    if k is None:
        continue
    cls, nxt = tables[k]
    st, forced = 0, 0
    for t in outs[v][0]:
        forced += int(cls[t]) >= 4
        st = int(nxt[st, cls[t]])
        assert st != 0xFFFF, v + ": a token that its state forbids"
    assert st == outs[v][2], v + ": the device's state is not the walk's"
    forced_share[v] = round(forced / n, 3)
assert not parent or outs["parent_spec"] == outs["plain_spec"], "this build's unconstrained stream or statistics are not the parent's"
tok_s = {v: [round(n / dt, 1) for dt in ts] for v, ts in secs.items()}
best = {v: max(x) for v, x in tok_s.items()}
steps = {v: (outs[v][1] if isinstance(outs[v][1], int) else outs[v][1][0]) for v in variants}
step_us = {v: [round(1e6 * dt / steps[v], 2) for dt in secs[v]] for v in variants if v.endswith("_spec")}
gain = [(forced_share["spec_T_" + k], best["spec_T_" + k] / best["sampled_" + k]) for k in shares]
break_even = None
if all(g >= 1 for _, g in gain):
    break_even = 0.0
else:
    for (x0, g0), (x1, g1) in zip(gain, gain[1:]):
        if g0 < 1 <= g1:
            break_even = round(x0 + (x1 - x0) * (1 - g0) / (g1 - g0), 3)
print(json.dumps({"model": name, "T": T, "parent_first": parent_first, "tokens": n, "reps": reps, "forced_share": forced_share, "steps": steps,
                  "tokens_per_step": {v: round(n / steps[v], 2) for v in variants}, "tok_s": tok_s, "best_tok_s": best,
                  "spec_over_sampled": {k: round(g, 3) for k, (_, g) in zip(shares, gain)}, "break_even_share": break_even,
                  "step_us": step_us, "step_spread_us": {v: round(max(x) - min(x), 2) for v, x in step_us.items()},
                  "plain_minus_parent_step_us": round(min(step_us["plain_spec"]) - min(step_us["parent_spec"]), 2) if parent else None}), flush=True)
sT.set_constraint(None)
s1.set_constraint(None)
for c in cons.values():
    be.constraint_free(c)
s1.close()
for which, (b, s) in side.items():
    use(which)
    s.close(), b.close()
mT.close(), m1.close()
