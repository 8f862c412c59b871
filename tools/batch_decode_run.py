"""Batched resident decode of one model: aggregate tok/s, ms per step and the plan's launch count per batch size, with the
multi-row K-on-lanes mat-vec (ZGML_HIP_OPT_SMALL_M_MATVEC) on and off, next to the single-sequence resident decode over the
same positions. One JSON line per (model, B, option, kv) with every repetition's figure; `reps` timed runs after one warm-up.

    timeout -k 10 300 python tools/batch_decode_run.py smollm-135m && timeout -k 10 900 python tools/batch_decode_run.py llama2-7b

(llama2-7b: all 32 layers, synthetic Q4_0 GGUF-valued weights, max_seq 512.) Positions [start, start + steps) = 4..132, the
range of profiles/r05_token_tail_ab.txt. Each run is a blocking call that ends with the tokens on the host; the clock is the
host's around it (128 graph launches: the launch of the call itself is < 1 % of a run).

Positional: model, batches ("4,8"), steps, start, reps. Flags, anywhere on the line:
  --kv-int8      every (B, option) is also run over per-sequence int8 KV caches (BatchModel kv_quant_block = 32), in the same
                 process, right after its f32-slab run ("kv": "f32" / "int8" in the line; int8 lines carry vs_f32)
  --admit N      before decoding, N tokens are prefilled on an f32 T-token plan of the same weights (in chunks of at most 128) and
                 every slot is admitted from it through zgml_hip_kv_move (BatchSession.admit); decoding then starts at position N
                 (or at `start`, where that is larger). The line carries the admission's time per slot, its bytes and GB/s, with non-temporal loads
                 (ZGML_HIP_OPT_KV_MOVE_NT) off and on; f32 lines also the whole-buffer zgml_hip_copy_program_buffer calls an f32
                 single-sequence hand-over takes for the same model
  --max-seq S    context length of the plans (default 512 for llama2-7b, else 2048)
  --options a,b  values of ZGML_HIP_OPT_SMALL_M_MATVEC to run (default 8,0)
  --no-single    skip the single-sequence reference run (vs_single is then left out)"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi, llama  # noqa: E402


def take_flag(args, name, has_value):
    if name not in args:
        return None
    i = args.index(name)
    value = args[i + 1] if has_value else True
    del args[i:i + (2 if has_value else 1)]
    return value


args = sys.argv[1:]
kv_int8 = bool(take_flag(args, "--kv-int8", False))
admit = int(take_flag(args, "--admit", True) or 0)
max_seq = int(take_flag(args, "--max-seq", True) or 0)
options = [int(o) for o in (take_flag(args, "--options", True) or "8,0").split(",")]
no_single = bool(take_flag(args, "--no-single", False))
name = args[0] if len(args) > 0 else "smollm-135m"
batches = [int(b) for b in args[1].split(",")] if len(args) > 1 else [1, 2, 4, 8]
steps = int(args[2]) if len(args) > 2 else 128
start = max(admit, int(args[3]) if len(args) > 3 else 4)
reps = int(args[4]) if len(args) > 4 else 3

be = Backend(0)
hip = capi.load_hip()
cfg = llama.preset(name, max_seq or (512 if name == "llama2-7b" else 2048))
assert start + steps <= cfg.max_seq_len, "positions beyond --max-seq"
m = llama.Model(cfg, llama.Q4_0, threads=16)
fns = llama.hip_backend_fns(be)


def launches(handle) -> int:
    return be.planText(handle).count("\n")


def emit(**kw):
    print(json.dumps({"model": name, "positions": [start, start + steps], **kw}), flush=True)


def kv_bytes_per_seq(block):
    """computed: bytes of one sequence's KV caches (f32 columns, or int8 bytes + one f32 scale per 32 dims)"""
    vals = 2 * cfg.n_layers * cfg.n_kv_heads * cfg.d_head * cfg.max_seq_len
    return vals * 4 if not block else vals + vals // block * 4


base_tps = None
if not no_single:  # the single-sequence resident decode (the existing decode plan) over the same positions
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

pre = pre_model = None
if admit:  # the prompt's caches: `admit` tokens through an f32 T-token plan, in chunks
    chunk = max(c for c in range(1, min(admit, 128) + 1) if admit % c == 0)
    pre_model = llama.Model(None, token_len=chunk, like=m)
    pre = llama.Session(pre_model, fns)
    prompt = [(31 * j + 7) % cfg.vocab_size for j in range(admit)]
    t0 = time.perf_counter()
    for p in range(0, admit, chunk):
        pre.prefill(prompt[p:p + chunk], p, want_logits=False)
    assert not be.last_error(), be.last_error()
    emit(path="prefill", tokens=admit, chunk=chunk, seconds=round(time.perf_counter() - t0, 4))


def timed_admits(bs, B, block):
    """every slot admitted from the prefill plan, non-temporal loads off and on: time per slot by the host clock around B calls and
    one synchronisation (best of reps), the host's share of it (the calls themselves, before the synchronisation: where that is
    well below the total the device was the limit), bytes moved per slot (read + written, computed) and GB/s"""
    lanes = 2 * cfg.n_layers * cfg.n_kv_heads
    vals = lanes * cfg.d_head * admit
    moved = vals * 4 + (vals * 4 if not block else vals + vals // block * 4)
    out = {"admit_cols": admit, "admit_lanes": lanes, "admit_bytes_per_slot": moved}
    for nt in (0, 1):
        be.set_option(capi.OPT_KV_MOVE_NT, nt)
        runs, host = [], []
        for _ in range(reps + 1):  # (the first repetition warms up)
            be.synchronize()
            t0 = time.perf_counter()
            for b in range(B):
                bs.admit(b, pre, admit)
            t1 = time.perf_counter()  # (the calls have returned: what the host spent enqueueing them)
            be.synchronize()
            runs.append((time.perf_counter() - t0) / B)
            host.append((t1 - t0) / B)
        best = min(runs[1:])
        out["admit_us_per_slot_nt%d" % nt] = round(best * 1e6, 1)
        out["admit_host_us_per_slot_nt%d" % nt] = round(min(host[1:]) * 1e6, 1)
        out["admit_gb_s_nt%d" % nt] = round(moved / best / 1e9, 1)
    be.set_option(capi.OPT_KV_MOVE_NT, 0)
    if not block:  # what the f32 hand-over of ONE sequence costs as whole-buffer copies between single-sequence plans' buffers
        pairs = list(zip(pre_model.kv_buffers(), bs.model.kv_buffers()))
        runs = []
        for _ in range(reps + 1):
            be.synchronize()
            t0 = time.perf_counter()
            for (sb, n), (db, _n) in pairs:
                assert hip.zgml_hip_copy_program_buffer(be.ctx, bs.handle, db, 0, pre.handle, sb, 0, n) == 0
            be.synchronize()
            runs.append(time.perf_counter() - t0)
        best = min(runs[1:])
        whole = sum(n for _b, n in pre_model.kv_buffers()) * 8
        out.update(copy_calls=len(pairs), copy_us=round(best * 1e6, 1), copy_bytes=whole, copy_gb_s=round(whole / best / 1e9, 1))
    assert not be.last_error(), be.last_error()
    return out


for B in batches:
    for on in options:  # (8: the row kernel at every B it is built for; the default value 1 stops at the measured bound, M <= 6)
        f32_best = None
        for block in ([0, 32] if kv_int8 else [0]):
            bs = llama.BatchSession(m, fns, B, small_m_matvec=on, kv_quant_block=block)
            extra = timed_admits(bs, B, block) if admit else {}
            if admit:
                for b in range(B):  # (the copies above went over slot 0: every slot holds the prompt when decoding starts)
                    bs.admit(b, pre, admit)
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
            best = B * steps / min(times)
            if not block:
                f32_best = best
            else:
                extra["vs_f32"] = round(best / f32_best, 3)
            if base_tps:
                extra["vs_single"] = round(best / base_tps, 3)
            emit(path="batch", B=B, option=on, kv="int8" if block else "f32", kv_bytes_per_seq=kv_bytes_per_seq(block), launches=text.count("\n") + 3,
                 rows_kernel_launches=text.count("qmatvec-kon-rows"), ms_per_step=[round(1e3 * t / steps, 4) for t in times],
                 tok_s=[round(B * steps / t, 1) for t in times], **extra)
            bs.close()
if pre:
    pre.close(), pre_model.close()
m.close()
be.close()
