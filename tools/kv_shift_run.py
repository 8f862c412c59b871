"""One context shift of a full KV cache (zgml_hip_kv_shift) against what a caller had to do before it existed: re-prefill the
kept tokens. One JSON line per invocation; run every figure in a fresh process.

    timeout -k 10 120 python tools/kv_shift_run.py shift smollm-135m f32
    timeout -k 10 120 python tools/kv_shift_run.py shift llama2-7b int8
    timeout -k 10 300 python tools/kv_shift_run.py prefill smollm-135m f32
    timeout -k 10 300 python tools/kv_shift_run.py prefill llama2-7b f32 --layers 2

shift:   the model's KV lanes at its dimensions (layers x kv heads x K | V lanes of max_seq columns of d_head) in holder programs
         — no weights are needed to move a cache, so Llama-2-7B's 2048 lanes are measured at full size —; keep 4,
         discard = (max_seq - keep) / 2, n_filled = max_seq; HIP events on the context stream around the one call; one warm-up, then
         5 repetitions: best, worst, and GB/s over the bytes read plus written (moved columns, scales included), from the best.
         The cache's contents are whatever the allocation holds (the kernel's work does not depend on the values).
prefill: resident_prefill of the max_seq - discard tokens that stay (rounded down to whole chunks) into a fresh T-token plan of
         the model, chunk tokens per launch sequence (default 128), host clock around the blocking calls, one warm-up pass, then
         3 passes: best and worst. --layers L builds the model with L layers only (Llama-2-7B's weights take minutes to
         synthesise): the line then carries the time scaled to the preset's layer count as `scaled_ms`, an extrapolation (the
         per-layer work is the same; the embedding gather and the LM head, which do not scale, are counted L_full / L times).

Flags: --max-seq S (default 2048), --keep K (default 4), --chunk T (default 128), --layers L."""
import ctypes as C
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
from zgml_amd import Backend, DeviceOp, DeviceProgram, capi, llama  # noqa: E402


def take_flag(args, name, default):
    if name not in args:
        return default
    i = args.index(name)
    value = int(args[i + 1])
    del args[i:i + 2]
    return value


args = sys.argv[1:]
max_seq, keep, chunk, layers = take_flag(args, "--max-seq", 2048), take_flag(args, "--keep", 4), take_flag(args, "--chunk", 128), take_flag(args, "--layers", 0)
mode, name, kv = args[0], args[1], args[2]
assert mode in ("shift", "prefill") and kv in ("f32", "int8")
cfg = llama.preset(name, max_seq)
full_layers = cfg.n_layers
discard = (max_seq - keep) // 2
n_move = max_seq - keep - discard
be = Backend(0)
hip = capi.load_hip()
out = {"mode": mode, "model": name, "kv": kv, "max_seq": max_seq, "keep": keep, "discard": discard, "d_head": cfg.d_head, "layers": full_layers,
       "kv_heads": cfg.n_kv_heads}

if mode == "shift":
    L, KV, dh, S = cfg.n_layers, cfg.n_kv_heads, cfg.d_head, max_seq
    if kv == "f32":  # the consolidated caches: one K and one V buffer per layer, a kv head's lane at kv * S * dh
        sizes = [KV * S * dh] * (2 * L)
        lanes = [(2 * l + w, k * S * dh, dh, S, 0) for l in range(L) for k in range(KV) for w in (0, 1)]
    else:  # one cache buffer per lane
        sizes = [S * dh // 4 + S * (dh // 32)] * (2 * L * KV)
        lanes = [(i, 0, dh, S, 32) for i in range(2 * L * KV)]
    n = len(sizes)
    h = be.compileProgram(DeviceProgram(ops=[DeviceOp.elementwise("add", n, i, i, 1) for i in range(n)], buffer_sizes=sizes + [1]))
    assert h, be.last_error()
    lanes_c = (capi.KvLaneC * len(lanes))(*[capi.KvLaneC(buf=b, d_head=d, n_cols=nc, block_size=bs, offset=off) for b, off, d, nc, bs in lanes])
    rotate = (C.c_uint8 * len(lanes))(*[1 - i % 2 for i in range(len(lanes))])
    ang = discard / (10000.0 ** (np.arange(dh // 2) * 2.0 / dh))
    c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    f32p = C.POINTER(C.c_float)
    rt = C.CDLL("libamdhip64.so")
    rt.hipEventCreate.argtypes, rt.hipEventRecord.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p, C.c_void_p]
    rt.hipEventSynchronize.argtypes, rt.hipEventElapsedTime.argtypes = [C.c_void_p], [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.zgml_hip_stream.restype, hip.zgml_hip_stream.argtypes = C.c_void_p, [C.c_void_p]
    stream = hip.zgml_hip_stream(be.ctx)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0
    ms = []
    for _ in range(6):  # (the first repetition warms up)
        assert rt.hipEventRecord(e0, stream) == 0
        rc = hip.zgml_hip_kv_shift(be.ctx, h, lanes_c, rotate, len(lanes), keep, discard, S, c.ctypes.data_as(f32p), s.ctypes.data_as(f32p))
        assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
        assert rc == 0 and not be.last_error(), be.last_error()
        t = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        ms.append(t.value)
    col_bytes = dh * 4 if kv == "f32" else dh + dh // 32 * 4
    moved = 2 * len(lanes) * n_move * col_bytes
    out.update(lanes=len(lanes), lane_bytes=S * col_bytes, moved_bytes=moved, warm_up_ms=round(ms[0], 4), best_ms=round(min(ms[1:]), 4),
               worst_ms=round(max(ms[1:]), 4), all_ms=[round(x, 4) for x in ms[1:]], gb_s=round(moved / (min(ms[1:]) * 1e-3) / 1e9, 1))
    be.freeProgram(h)
else:
    if layers:
        cfg.n_layers = layers
    cfg.kv_quant_block = 32 if kv == "int8" else 0
    n_kept = (max_seq - discard) // chunk * chunk
    m = llama.Model(cfg, llama.Q4_0, threads=16, token_len=chunk)
    s = llama.Session(m, llama.hip_backend_fns(be))
    s.resident_setup(be)
    toks = [(31 * j + 7) % cfg.vocab_size for j in range(n_kept)]
    secs = []
    for _ in range(4):  # (the first pass warms up)
        be.synchronize()
        t0 = time.perf_counter()
        for p in range(0, n_kept, chunk):
            s.resident_prefill(toks[p:p + chunk], p)
        be.synchronize()
        secs.append(time.perf_counter() - t0)
    assert not be.last_error(), be.last_error()
    out.update(tokens=n_kept, chunk=chunk, built_layers=cfg.n_layers, warm_up_ms=round(secs[0] * 1e3, 3), best_ms=round(min(secs[1:]) * 1e3, 3),
               worst_ms=round(max(secs[1:]) * 1e3, 3))
    if cfg.n_layers != full_layers:
        out["scaled_ms"] = round(min(secs[1:]) * 1e3 * full_layers / cfg.n_layers, 3)
    s.close(), m.close()
print(json.dumps(out), flush=True)
be.close()
