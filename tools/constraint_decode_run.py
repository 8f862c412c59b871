"""What constrained decoding (a token automaton masks the sampled picks on the device: zgml_token_dfa, include/zgml_hip.h) costs in
the sampled resident loop, and that a call without a constraint costs what it did: µs per token of
    constrained       zgml_hip_resident_decode_sampled with an automaton of 5 states and 7 classes attached (about 40 % of the
                      transitions forbidden, no state without a token)
    constrained_8192  ... with 8192 classes, the widest state row (16 KiB staged per workgroup)
    constrained_pen   ... the first automaton with repeat_penalty 1.1 over the last 64 tokens as well
    plain             the same loop with nothing attached, this build
    parent            the same loop of ANOTHER build of the library — the parent commit's, given as argv[4] — on a context and a
                      program of its own over the same weights
all in one process, alternating inside every repetition, one untimed run of each first (graph capture). One JSON line; every
repetition's figure is kept, `spread_us` is the largest difference between two repetitions of one variant.

    timeout -k 10 300 python tools/constraint_decode_run.py smollm-135m 200 5 /path/to/parent/libzgml_hip.so

    argv: preset [steps = 200] [reps = 5] [parent library = none] [start position = 8]

(llama2-7b: all 32 layers, synthetic Q4_0 weights, max_seq 512.) Each timed run is a blocking call that ends with the tokens on
the host; the clock is the host's around it, and attaching the automaton (a blocking upload of a few words) lies outside it.
Checked as well: plain and parent give the same tokens, every constrained token is allowed in the state it was picked in, and
the device's final state is the one the tokens lead to."""
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
V = cfg.vocab_size
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


def automaton(seed, n_states, n_classes):
    """class_of a hash of the index; about 40 % of the transitions forbidden, every state keeps an allowed class"""
    rng = np.random.default_rng(seed)
    i = np.arange(V, dtype=np.uint64)
    cls = (((i * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(n_classes)).astype(np.uint16)
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(np.uint16)
    nxt[rng.random((n_states, n_classes)) < 0.4] = 0xFFFF
    for st in range(n_states):
        if np.all(nxt[st] == 0xFFFF):
            nxt[st, st % n_classes] = (st + 1) % n_states
    return cls, nxt


use("this")
be, sess = side["this"]
tables = {"small": automaton(1, 5, 7), "wide": automaton(2, 5, 8192)}
cons = {k: be.constraint_create(*t) for k, t in tables.items()}
base = dict(temperature=0.8, top_k=40, top_p=0.95, seed=1)
S = capi.SamplingC.of
plain_sp, pen_sp = S(**base), S(**base, repeat_penalty=1.1, penalty_window=64, recent=history)
# variant -> (library, automaton or None, parameters)
variants = {"constrained": ("this", "small", plain_sp), "constrained_8192": ("this", "wide", plain_sp), "constrained_pen": ("this", "small", pen_sp),
            "plain": ("this", None, plain_sp)}
if parent:
    variants["parent"] = ("parent", None, plain_sp)

secs, toks, finals = {k: [] for k in variants}, {}, {}
for rep in range(reps + 1):  # (rep 0: untimed)
    for k, (which, table, sp) in variants.items():
        use(which)
        if which == "this":
            sess.set_constraint(cons[table] if table else None, 0)
        t0 = time.perf_counter()
        out = side[which][1].resident_decode_sampled(first, start, steps, sp)[0].tolist()
        dt = time.perf_counter() - t0
        assert toks.setdefault(k, out) == out, k + ": a repetition produced other tokens"
        if which == "this":
            finals[k] = sess.constraint_state()
        if rep:
            secs[k].append(dt)
use("this")
sess.set_constraint(None)
for c in cons.values():
    be.constraint_free(c)
for which, (b, _) in side.items():
    assert not b.last_error(), b.last_error()
for k, (which, table, sp) in variants.items():  # every constrained token is allowed where it was picked; the state is the walk's
    if not table:
        continue
    cls, nxt = tables[table]
    st = 0
    for t in toks[k]:
        st = int(nxt[st, cls[t]])
        assert st != 0xFFFF, k + ": a token that its state forbids"
    assert st == finals[k], k + ": the device's state is not the walk's"
assert finals["plain"] == -1
assert not parent or toks["parent"] == toks["plain"], "this build's unconstrained stream is not the parent's"
us = {k: [round(1e6 * dt / steps, 2) for dt in v] for k, v in secs.items()}
print(json.dumps({"model": name, "steps": steps, "start": start, "reps": reps, **base, "us_per_token": us,
                  "best_us": {k: min(v) for k, v in us.items()}, "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()},
                  "constrained_more_us": round(min(us["constrained"]) - min(us["plain"]), 2),
                  "constrained_8192_more_us": round(min(us["constrained_8192"]) - min(us["plain"]), 2),
                  "constrained_pen_more_us": round(min(us["constrained_pen"]) - min(us["plain"]), 2),
                  "plain_minus_parent_us": round(min(us["plain"]) - min(us["parent"]), 2) if parent else None,
                  "constrained_differs_from_plain": toks["constrained"] != toks["plain"],
                  "distinct_tokens": {k: len(set(v)) for k, v in toks.items()}}), flush=True)
for which, (b, s) in side.items():
    use(which)
    s.close(), b.close()
m.close()
