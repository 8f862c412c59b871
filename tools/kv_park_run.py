"""Parking a sequence's KV columns in host memory and resuming them (zgml_hip_kv_park / zgml_hip_kv_resume) against the two routes
a caller had before: one zgml_program_io per lane run through zgml_hip_download_outputs / zgml_hip_upload_inputs, and re-prefilling
the same tokens. One JSON line per invocation; run every figure in a fresh process. The two older routes exist in an older build
too: load it through ZGML_HIP_LIB to measure them there.

    timeout -k 10 120 python tools/kv_park_run.py park smollm-135m f32 --cols 256
    timeout -k 10 120 python tools/kv_park_run.py park llama2-7b f32 --cols 2048 --int8
    timeout -k 10 120 python tools/kv_park_run.py park llama2-7b int8 --cols 16
    timeout -k 10 120 python tools/kv_park_run.py lanes llama2-7b f32 --cols 2048
    timeout -k 10 300 python tools/kv_park_run.py prefill smollm-135m f32 --cols 256
    timeout -k 10 300 python tools/kv_park_run.py prefill llama2-7b f32 --cols 2048 --layers 2

park:    the lanes of ONE sequence at the model's dimensions (layers x kv heads x K | V lanes of max_seq columns of d_head) in a
         holder program — f32: the single-sequence plan's consolidated caches; int8: one slot of an int8 batched plan, a cache
         buffer per lane; no weights are needed to move a cache, so Llama-2-7B's 2048 lanes are measured at full size. Columns
         [0, cols). Host clock around the call: a park blocks until the blob is complete; a resume is followed by a synchronise
         (its unpack launch is stream-ordered), so the figure is call plus launch. Two warm-up calls (staging allocation, first
         launch), then 9: median, best, worst, and GB/s of the blob over the median. --int8: ZGML_KV_PARK_INT8 (f32 lanes only).
         The blob is ordinary pageable memory, as an application's would be.
lanes:   the same columns through one zgml_program_io per lane run (int8: two, bytes and scales) in one
         zgml_hip_download_outputs call, and back through one zgml_hip_upload_inputs call plus a synchronise; same repetitions.
prefill: resident_prefill of `cols` tokens into a fresh T-token plan of the model (chunks of min(cols, --chunk)), host clock
         around the blocking calls, one warm-up pass, then 3: median, best, worst. --layers L builds L layers only (Llama-2-7B's
         weights take minutes to synthesise) and adds `scaled_ms`, the time scaled to the preset's layer count: an extrapolation.

Flags: --cols N (default 2048), --max-seq S (default 2048), --chunk T (default 128), --layers L, --int8."""
import json
import statistics
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
from zgml_amd import Backend, DeviceOp, DeviceProgram, ProgramIO, capi, llama  # noqa: E402
from zgml_amd.program import ios_to_c  # noqa: E402


def take_flag(args, name, default):
    if name not in args:
        return default
    i = args.index(name)
    value = int(args[i + 1])
    del args[i:i + 2]
    return value


def timed(fn, warm, reps):
    """-> milliseconds of `reps` calls after `warm` untimed ones; fn ends in a device synchronise"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def figures(prefix, ms, nbytes=None):
    med = statistics.median(ms)
    d = {prefix + "_ms": round(med, 4), prefix + "_best_ms": round(min(ms), 4), prefix + "_worst_ms": round(max(ms), 4)}
    if nbytes:
        d[prefix + "_gb_s"] = round(nbytes / (med * 1e-3) / 1e9, 2)
    return d


args = sys.argv[1:]
int8_flag = "--int8" in args
if int8_flag:
    args.remove("--int8")
cols, max_seq, chunk, layers = take_flag(args, "--cols", 2048), take_flag(args, "--max-seq", 2048), take_flag(args, "--chunk", 128), take_flag(args, "--layers", 0)
mode, name, kv = args[0], args[1], args[2]
assert mode in ("park", "lanes", "prefill") and kv in ("f32", "int8") and 0 < cols <= max_seq
cfg = llama.preset(name, max_seq)
full_layers = cfg.n_layers
be = Backend(0)
hip = capi.load_hip()
out = {"mode": mode, "model": name, "kv": kv, "cols": cols, "max_seq": max_seq, "d_head": cfg.d_head, "layers": full_layers, "kv_heads": cfg.n_kv_heads}

if mode in ("park", "lanes"):
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
    out["lanes"] = len(lanes)
    if mode == "park":
        lanes_c = (capi.KvLaneC * len(lanes))(*[capi.KvLaneC(buf=b, d_head=d, n_cols=nc, block_size=bs, offset=off) for b, off, d, nc, bs in lanes])
        flags = capi.KV_PARK_INT8 if int8_flag else 0
        size = int(hip.zgml_hip_kv_park_bytes(lanes_c, len(lanes), cols, flags))
        assert size, "refused lane table"
        blob = np.zeros(size, np.uint8)

        def park():
            assert hip.zgml_hip_kv_park(be.ctx, h, lanes_c, len(lanes), 0, cols, flags, blob.ctypes.data, size) == 0, be.last_error()

        out.update(int8_flag=int8_flag, blob_bytes=size, **figures("park", timed(park, 2, 9), size))
        if not (int8_flag and kv == "f32"):  # (a quantised blob of f32 lanes resumes into int8 plans only)
            def resume():
                assert hip.zgml_hip_kv_resume(be.ctx, h, lanes_c, len(lanes), 0, blob.ctypes.data, size) == 0, be.last_error()
                be.synchronize()

            out.update(figures("resume", timed(resume, 2, 9), size))
    else:
        ios, keep = [], []
        for b, off, d, nc, bs in lanes:  # (offsets and sizes in bytes)
            runs = [(off * 4, cols * d * 4)] if not bs else [(0, cols * d), (nc * d, cols * (d // 32) * 4)]
            for o, sz in runs:
                host = np.zeros(sz, np.uint8)
                keep.append(host)
                ios.append(ProgramIO(b, host, offset=o, size=sz))
        ios_c = ios_to_c(ios)
        nbytes = sum(a.nbytes for a in keep)

        def down():
            hip.zgml_hip_download_outputs(be.ctx, h, ios_c, len(ios))

        def up():
            hip.zgml_hip_upload_inputs(be.ctx, h, ios_c, len(ios))
            be.synchronize()

        out.update(ios=len(ios), bytes=nbytes, **figures("download", timed(down, 2, 9), nbytes), **figures("upload", timed(up, 2, 9), nbytes))
    assert not be.last_error(), be.last_error()
    be.freeProgram(h)
else:
    if layers:
        cfg.n_layers = layers
    cfg.kv_quant_block = 32 if kv == "int8" else 0
    T = min(cols, chunk)
    n_tok = cols // T * T
    m = llama.Model(cfg, llama.Q4_0, threads=16, token_len=T)
    s = llama.Session(m, llama.hip_backend_fns(be))
    s.resident_setup(be)
    toks = [(31 * j + 7) % cfg.vocab_size for j in range(n_tok)]

    def prefill():
        for p in range(0, n_tok, T):
            s.resident_prefill(toks[p:p + T], p)
        be.synchronize()

    ms = timed(prefill, 1, 3)
    assert not be.last_error(), be.last_error()
    out.update(tokens=n_tok, chunk=T, built_layers=cfg.n_layers, **figures("prefill", ms))
    if cfg.n_layers != full_layers:
        out["scaled_ms"] = round(statistics.median(ms) * full_layers / cfg.n_layers, 3)
    s.close(), m.close()
print(json.dumps(out), flush=True)
be.close()
