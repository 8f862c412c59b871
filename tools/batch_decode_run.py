"""Batched resident decode of one model: aggregate tok/s, ms per step and the plan's launch count per batch size, with the
multi-row K-on-lanes mat-vec (ZGML_HIP_OPT_SMALL_M_MATVEC) on and off, next to the single-sequence resident decode over the
same positions. One JSON line per (model, B, option) with every repetition's figure; `reps` timed runs after one warm-up.

    timeout -k 10 300 python tools/batch_decode_run.py smollm-135m && timeout -k 10 900 python tools/batch_decode_run.py llama2-7b

(llama2-7b: all 32 layers, synthetic Q4_0 GGUF-valued weights, max_seq 512.) Positions [start, start + steps) = 4..132, the
range of profiles/r05_token_tail_ab.txt. Each run is a blocking call that ends with the tokens on the host; the clock is the
host's around it (128 graph launches: the launch of the call itself is < 1 % of a run)."""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "smollm-135m"
batches = [int(b) for b in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 2, 4, 8]
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 128
start = int(sys.argv[4]) if len(sys.argv) > 4 else 4
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3

be = Backend(0)
hip = capi.load_hip()
cfg = llama.preset(name, 512 if name == "llama2-7b" else 2048)
m = llama.Model(cfg, llama.Q4_0, threads=16)
fns = llama.hip_backend_fns(be)


def launches(handle) -> int:
    return be.planText(handle).count("\n")


def emit(**kw):
    print(json.dumps({"model": name, "positions": [start, start + steps], **kw}), flush=True)


# the single-sequence resident decode (the existing decode plan) over the same positions
s = llama.Session(m, fns)
s.resident_setup(be)
w = s.resident_decode(1, 0, 4)
s.resident_decode(int(w[-1]), start, steps)  # warm-up
single = []
for _ in range(reps):
    t0 = time.perf_counter()
    s.resident_decode(int(w[-1]), start, steps)
    single.append(time.perf_counter() - t0)
assert not be.last_error(), be.last_error()
base_tps = steps / min(single)
emit(path="single", B=1, option=None, launches=launches(s.handle) + 3, ms_per_step=[round(1e3 * t / steps, 4) for t in single],
     tok_s=[round(steps / t, 1) for t in single])
s.close()

for B in batches:
    for on in (8, 0):  # (8: the row kernel at every B it is built for; the default value 1 stops at the measured bound, M <= 6)
        bs = llama.BatchSession(m, fns, B, small_m_matvec=on)
        bs.resident_setup(be)
        first = [(911 * b + 17) % cfg.vocab_size for b in range(B)]
        bs.resident_decode_batch(first, [start] * B, steps)  # warm-up (captures the graph)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            toks = bs.resident_decode_batch(first, [start] * B, steps)
            times.append(time.perf_counter() - t0)
        assert not be.last_error(), be.last_error()
        assert toks.shape == (B, steps) and (toks >= 0).all()
        text = be.planText(bs.handle)
        emit(path="batch", B=B, option=on, launches=text.count("\n") + 3, rows_kernel_launches=text.count("qmatvec-kon-rows"),
             ms_per_step=[round(1e3 * t / steps, 4) for t in times], tok_s=[round(B * steps / t, 1) for t in times],
             vs_single=round(B * steps / min(times) / base_tps, 3))
        bs.close()
m.close()
be.close()
