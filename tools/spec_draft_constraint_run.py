"""What the masked draft costs and gives (zgml_hip_resident_decode_speculative_model_constrained, include/zgml_hip.h), per model at T = 4:

  cost    µs per verify step that ran of the new call under an automaton that allows EVERY token — 7 hashed classes, and 8192 (a
          16 KiB state row staged by every workgroup of the T masked stage-1 launches) — against
          zgml_hip_resident_decode_speculative_model with the same sampling set on the same pair: the same tokens and steps
          (asserted), so the difference is the class gather and the row staging of the masked launches alone.
  gain    tokens per step under the tests' TEMPLATE and SEEDED automata (scaled to the model's vocabulary) with the mask — the
          device call's statistics — and WITHOUT it: the host-driven loop of tests/spec_draft_constraint_model.py with mask=False
          on the same plans (no device call drafts unmasked under a constraint). The streams are equal (asserted).

    timeout -k 10 300 python tools/spec_draft_constraint_run.py smollm-135m 2 && \
    timeout -k 10 600 python tools/spec_draft_constraint_run.py llama2-7b 1 --layers 2

Positional: model, the draft's layer count (the target's dimensions), tokens, reps. --layers L: a target of L layers of the model's
dimensions (the masked launches' cost does not depend on the layers). Synthetic Q4_0 weights: the tokens per step are those of
two unrelated synthetic models and say nothing about trained ones. Each run is a blocking call that ends with the tokens on the
host; the clock is the host's around it, best of `reps` after one warm-up (which also captures the graph); the calls alternate."""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
from zgml_amd import Backend, capi, llama  # noqa: E402
from tests import spec_constraint_model as SCM  # noqa: E402
from tests import spec_draft_constraint_model as SDM  # noqa: E402
from tests.test_constraint_host import Dfa, c_constraint_sample  # noqa: E402
from tests.test_hip_constraint import hashed_classes, seeded_dfa  # noqa: E402
from tests.test_spec_constraint_host import template_dfa  # noqa: E402

args = sys.argv[1:]
layers = None
if "--layers" in args:
    i = args.index("--layers")
    layers = int(args[i + 1])
    del args[i:i + 2]
name = args[0] if len(args) > 0 else "smollm-135m"
draft_layers = int(args[1]) if len(args) > 1 else 2
tokens = int(args[2]) if len(args) > 2 else 96
reps = int(args[3]) if len(args) > 3 else 5
T, FIRST, MAX_SEQ = 4, 17, 256
S = capi.SamplingC.of
sp = S(0.8, 40, 0.95, seed=7, stream=0)

be = Backend(0)
fns = llama.hip_backend_fns(be)


def cfg_of(n_layers):
    cfg = llama.preset(name, MAX_SEQ)
    if n_layers is not None:
        cfg.n_layers = n_layers
    return cfg


def session(model, small_m=None, setup=True):
    if small_m is not None:
        be.set_option(capi.OPT_SMALL_M_MATVEC, small_m)
    try:
        s = llama.Session(model, fns)
    finally:
        be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
    if setup:
        s.resident_setup(be)
    return s


vocab = cfg_of(layers).vocab_size
tm = llama.Model(cfg_of(layers), llama.Q4_0, threads=16, token_len=T)
dm = llama.Model(cfg_of(draft_layers), llama.Q4_0, threads=16)
ts, ds = session(tm, small_m=1), session(dm)


def steps_of(call):
    before = int(be.getRuntimeProfile(ts.handle).call_count)
    out = call()
    return int(be.getRuntimeProfile(ts.handle).call_count) - before, out


def timed(calls):
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


def constrained(c, state, n=tokens):
    ts.set_constraint(c, state)
    return ts.resident_decode_speculative_model_constrained(ds, FIRST, 0, n, sp)


# ── cost ──
ts.set_constraint(None)
steps_plain, plain = steps_of(lambda: ts.resident_decode_speculative_model(ds, FIRST, 0, tokens, sampling=sp))
for n_classes in (7, 8192):
    every = be.constraint_create(hashed_classes(vocab, n_classes), np.zeros((1, n_classes), np.uint16))
    steps, got = steps_of(lambda: constrained(every, 0))
    assert (got[0].tolist(), got[1], got[2]) == (plain[0].tolist(), plain[1], plain[2]) and steps == steps_plain  # the mask allows everything

    def parent_call():
        ts.set_constraint(None)
        ts.resident_decode_speculative_model(ds, FIRST, 0, tokens, sampling=sp)

    t_con, t_plain = timed([lambda: constrained(every, 0), parent_call])
    row = dict(model=name, target_layers=layers, draft_layers=draft_layers, vocab=vocab, T=T, n_classes=n_classes, tokens=tokens, steps_run=steps,
               t_step_constrained_us=round(1e6 * t_con / steps, 2), t_step_model_us=round(1e6 * t_plain / steps, 2))
    row["delta_us_per_step"] = round(row["t_step_constrained_us"] - row["t_step_model_us"], 2)
    print(json.dumps(row), flush=True)
    ts.set_constraint(None)
    be.constraint_free(every)

# ── gain ── (the reference plans are the device pair's own, driven through the vtable)
n_gain = min(tokens, 48)


def host_loop(dfa, state, mask):
    def rows(c, pos, row_state, known):
        ts.prefill(c, pos, want_logits=False)
        logits = np.zeros((T, vocab), np.float32)
        io = (capi.ProgramIOC * 1)(capi.ProgramIOC(tm.buf("logits"), 0, 0, logits.ctypes.data, 4 * T * vocab, 0))
        capi.load_hip().zgml_hip_download_outputs(be.ctx, ts.handle, io, 1)
        g = []
        for j in range(T):
            tok = -1 if row_state[j] == SCM.DEAD else c_constraint_sample(logits[j], sp, pos + j, None, dfa, row_state[j])[0]
            g.append(tok if tok >= 0 else SCM.NO_PICK)
        return g
    return SDM.spec_loop(rows, lambda tok, pos: ds.step(tok, pos)[1], FIRST, 0, n_gain, T, dfa.class_of, dfa.next, state, mask=mask)


for label, dfa, state in (("template", template_dfa(vocab, [0, 1, 0, 3, 0, 6], seed=21)[0], 0), ("seeded", seeded_dfa(11, vocab), 1)):
    c = be.constraint_create(dfa.class_of, dfa.next)
    toks, produced, stats = constrained(c, state, n_gain)
    ts.set_constraint(None)
    masked, unmasked = host_loop(dfa, state, True), host_loop(dfa, state, False)
    assert masked[0] == unmasked[0] == toks.tolist() and masked[2] == stats, (masked[2], stats)  # drafts never change tokens; the device is the model's loop
    print(json.dumps(dict(model=name, automaton=label, tokens=produced, masked=stats, unmasked=unmasked[2],
                          tokens_per_step_masked=round(produced / stats["steps"], 3), tokens_per_step_unmasked=round(unmasked[1] / unmasked[2]["steps"], 3))), flush=True)
    be.constraint_free(c)

print(f"\n{name}: T = {T}, {tokens} tokens from position 0, best of {reps}; synthetic Q4_0 weights (tokens per step on trained weights: not measured)")
for x in (ts, tm, ds, dm):
    x.close()
be.close()
