"""Python binding of the C++ host side (zgml_amd/host): synthetic LLaMA models, the decode
DeviceProgram (DeviceInference lowering) and the per-token session loop. The compute backend is a
function table with the zgml_hip_* signatures — the HIP library in the product, the oracle's
`zo_vt_*` wrappers in tests."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import capi

Q4_0, Q8_0, F32_DENSE, Q4_0_GGUF = 0, 1, 2, 3


class Config(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("vocab_size", "d_model", "n_heads", "n_kv_heads", "d_ff", "n_layers",
                                           "max_seq_len")] + [
        ("rope_base", C.c_float), ("rms_norm_eps", C.c_float), ("tied_lm_head", C.c_uint32),
        ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32), ("kv_quant_block", C.c_uint32)]

    @property
    def d_head(self):
        return self.d_model // self.n_heads


class BackendFns(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("compile_program", C.c_void_p), ("refresh_program", C.c_void_p),
                ("execute_program", C.c_void_p), ("free_program", C.c_void_p)]


class GatherPoint(C.Structure):
    _fields_ = [("op_end", C.c_uint32), ("buf", C.c_uint16), ("_pad", C.c_uint16), ("offset", C.c_uint32),
                ("len_per_rank", C.c_uint32)]


_lib = None


def load_host() -> C.CDLL:
    global _lib
    if _lib is None:
        path = capi.HOST_LIB_PATH
        if not Path(path).exists():
            raise RuntimeError(f"{path} not found: run __graft_entry__.build()")
        lib = C.CDLL(str(path))
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.zh_preset.argtypes, lib.zh_preset.restype = [C.c_char_p, u32, C.POINTER(Config)], None
        lib.zh_model_create.argtypes, lib.zh_model_create.restype = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int], vp
        lib.zh_model_create_ex.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int, u32]
        lib.zh_model_create_ex.restype = vp
        lib.zh_model_create_like.argtypes, lib.zh_model_create_like.restype = [vp, C.c_int, C.c_int, u32], vp
        lib.zh_model_patch_tokens.argtypes, lib.zh_model_patch_tokens.restype = [vp, vp, u32], None
        lib.zh_session_prefill.argtypes, lib.zh_session_prefill.restype = [vp, vp, u32, vp], C.c_int64
        lib.zh_model_free.argtypes, lib.zh_model_free.restype = [vp], None
        lib.zh_model_program.argtypes, lib.zh_model_program.restype = [vp], C.POINTER(capi.DeviceProgramC)
        lib.zh_model_patch.argtypes, lib.zh_model_patch.restype = [vp, u32, u32], None
        lib.zh_model_step_inputs.argtypes, lib.zh_model_step_inputs.restype = [vp, C.POINTER(u64)], C.POINTER(capi.ProgramIOC)
        lib.zh_model_step_outputs.argtypes, lib.zh_model_step_outputs.restype = [vp, C.POINTER(u64)], C.POINTER(capi.ProgramIOC)
        lib.zh_model_logits.argtypes, lib.zh_model_logits.restype = [vp], C.POINTER(C.c_float)
        lib.zh_model_token_embed.argtypes, lib.zh_model_token_embed.restype = [vp], C.POINTER(C.c_float)
        lib.zh_model_rope_table.argtypes, lib.zh_model_rope_table.restype = [vp, C.c_int], C.POINTER(C.c_float)
        lib.zh_model_buf.argtypes, lib.zh_model_buf.restype = [vp, C.c_int, u32], C.c_uint16
        lib.zh_model_gather_points.argtypes, lib.zh_model_gather_points.restype = [vp, C.POINTER(GatherPoint), u64], u64
        lib.zh_model_kv_buffers.argtypes = [vp, C.POINTER(C.c_uint16), C.POINTER(u64), u64]
        lib.zh_model_kv_buffers.restype = u64
        lib.zh_model_quant_bytes.argtypes, lib.zh_model_quant_bytes.restype = [vp, C.POINTER(u64)], u64
        lib.zh_session_create.argtypes, lib.zh_session_create.restype = [vp, C.POINTER(BackendFns)], vp
        lib.zh_session_free.argtypes, lib.zh_session_free.restype = [vp], None
        lib.zh_session_handle.argtypes, lib.zh_session_handle.restype = [vp], vp
        lib.zh_session_step.argtypes, lib.zh_session_step.restype = [vp, u32, u32, vp], C.c_int64
        lib.zh_session_decode.argtypes, lib.zh_session_decode.restype = [vp, u32, u32, u32, vp], C.c_double
        lib.zh_session_set_refresh_dynamic.argtypes, lib.zh_session_set_refresh_dynamic.restype = [vp, vp], None
        lib.zh_model_create_batch.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int, u32, C.c_char_p, u64]
        lib.zh_model_create_batch.restype = vp
        lib.zh_model_create_batch_like.argtypes = [vp, C.c_int, C.c_int, u32, C.c_char_p, u64]
        lib.zh_model_create_batch_like.restype = vp
        lib.zh_model_create_batch_kvq.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int, u32, u32, C.c_char_p, u64]
        lib.zh_model_create_batch_kvq.restype = vp
        lib.zh_model_create_batch_like_kvq.argtypes = [vp, C.c_int, C.c_int, u32, u32, C.c_char_p, u64]
        lib.zh_model_create_batch_like_kvq.restype = vp
        lib.zh_model_create_batch_ts.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int, u32, u32, u32, C.c_char_p, u64]
        lib.zh_model_create_batch_ts.restype = vp
        lib.zh_model_create_batch_like_ts.argtypes = [vp, C.c_int, C.c_int, u32, u32, u32, C.c_char_p, u64]
        lib.zh_model_create_batch_like_ts.restype = vp
        lib.zh_model_tokens_per_seq.argtypes, lib.zh_model_tokens_per_seq.restype = [vp], u32
        lib.zh_model_kv_lanes.argtypes, lib.zh_model_kv_lanes.restype = [vp, C.POINTER(capi.KvLaneC), u64], u64
        lib.zh_model_n_seqs.argtypes, lib.zh_model_n_seqs.restype = [vp], u32
        lib.zh_model_patch_batch.argtypes, lib.zh_model_patch_batch.restype = [vp, vp, vp], None
        lib.zh_model_dyn_sequences.argtypes, lib.zh_model_dyn_sequences.restype = [vp, C.POINTER(u32), C.POINTER(u32), u64], u64
        lib.zh_session_set_refresh_dynamic_batch.argtypes, lib.zh_session_set_refresh_dynamic_batch.restype = [vp, vp], None
        lib.zh_session_step_batch.argtypes, lib.zh_session_step_batch.restype = [vp, vp, vp, vp, vp], C.c_int
        lib.zh_argmax.argtypes, lib.zh_argmax.restype = [vp, u32], u32
        lib.zh_argmax_reference.argtypes, lib.zh_argmax_reference.restype = [vp, u32], u32
        _lib = lib
    return _lib


def preset(name: str, max_seq: int = 0) -> Config:
    c = Config()
    load_host().zh_preset(name.encode(), max_seq, C.byref(c))
    return c


def _fn_addr(lib, name) -> int:
    return C.cast(getattr(lib, name), C.c_void_p).value


def hip_backend_fns(backend) -> BackendFns:
    """Function table of the HIP library for context `backend.ctx` (zgml_amd.Backend)."""
    lib = capi.load_hip()
    return BackendFns(backend.ctx, _fn_addr(lib, "zgml_hip_compile_program"), _fn_addr(lib, "zgml_hip_refresh_program"),
                      _fn_addr(lib, "zgml_hip_execute_program"), _fn_addr(lib, "zgml_hip_free_program"))


class Model:
    """Synthetic LLaMA weights + the decode DeviceProgram (`DeviceInference.init`, token_len = 1)."""

    n_seqs = 0  # (BatchModel: sequences per step)

    def __init__(self, cfg: Config, weight_kind: int = Q4_0, fused_elementwise: bool = True,
                 include_dead_f32: bool = False, threads: int = 8, token_len: int = 1, like: "Model" = None):
        """`like`: build the plan over that model's weights (shared, not generated again; cfg / weight_kind come from it, and it
        must outlive this one's sessions): e.g. the T-token prefill plan beside a decode or batched plan."""
        self.lib = load_host()
        self.cfg = like.cfg if like else cfg
        self.token_len = token_len
        if like:
            self.build_args = like.build_args
            self.ptr = self.lib.zh_model_create_like(like.ptr, int(like.build_args[1]), int(like.build_args[2]), token_len)
        else:
            self.build_args = (weight_kind, fused_elementwise, include_dead_f32, threads)
            self.ptr = self.lib.zh_model_create_ex(C.byref(cfg), weight_kind, int(fused_elementwise), int(include_dead_f32),
                                                   threads, token_len)
        if not self.ptr:
            raise ValueError("invalid LlamaConfig / shard spec")

    def close(self):
        if self.ptr:
            self.lib.zh_model_free(self.ptr)
            self.ptr = None

    @property
    def program(self) -> capi.DeviceProgramC:
        return self.lib.zh_model_program(self.ptr).contents

    def patch(self, token: int, pos: int) -> None:
        self.lib.zh_model_patch(self.ptr, token, pos)

    def buf(self, which: str, layer: int = 0) -> int:
        idx = {"token_input": 0, "attn_mask": 1, "logits": 2, "rope": 3, "k_cache": 4, "v_cache": 5}[which]
        return int(self.lib.zh_model_buf(self.ptr, idx, layer))

    def token_embed(self) -> np.ndarray:
        p = self.lib.zh_model_token_embed(self.ptr)
        return np.ctypeslib.as_array(p, shape=(self.cfg.vocab_size, self.cfg.d_model))

    def rope_tables(self):
        shape = (self.cfg.max_seq_len, self.cfg.d_head)
        return (np.ctypeslib.as_array(self.lib.zh_model_rope_table(self.ptr, 0), shape=shape),
                np.ctypeslib.as_array(self.lib.zh_model_rope_table(self.ptr, 1), shape=shape))

    def gather_points(self):
        n = self.lib.zh_model_gather_points(self.ptr, None, 0)
        arr = (GatherPoint * max(1, n))()
        self.lib.zh_model_gather_points(self.ptr, arr, n)
        return list(arr[:n])

    def kv_buffers(self):
        """[(buffer id, f32 elements)] of every KV-cache buffer, in builder order (same order in a prefill plan and the
        decode plan of one config: the hand-off of llama_inference.prefill -> step is a pairwise copy)."""
        n = self.lib.zh_model_kv_buffers(self.ptr, None, None, 0)
        bufs, elems = (C.c_uint16 * max(1, n))(), (C.c_uint64 * max(1, n))()
        self.lib.zh_model_kv_buffers(self.ptr, bufs, elems, n)
        return [(int(bufs[i]), int(elems[i])) for i in range(n)]

    def kv_lanes(self, seq: int = None):
        """capi.KvLaneC array of the plan's KV lanes (DecodeProgram::kv_lanes): one per (sequence, layer, kv head, K | V), in that
        nesting order; `seq`: that sequence's lanes only. Lane i of two plans of one config is the same head's cache, whatever
        the plans' forms (decode, T-token, batched; f32 or int8): what Backend-level zgml_hip_kv_move takes."""
        cache = self.__dict__.setdefault("_kv_lanes", {})  # (a plan's lanes never change: built once per sequence asked for)
        if seq in cache:
            return cache[seq]
        n = self.lib.zh_model_kv_lanes(self.ptr, None, 0)
        arr = (capi.KvLaneC * max(1, n))()
        self.lib.zh_model_kv_lanes(self.ptr, arr, n)
        if seq is None:
            cache[seq] = (capi.KvLaneC * n)(*arr[:n])
            return cache[seq]
        per = n // max(1, self.n_seqs)
        if not 0 <= seq < max(1, self.n_seqs):
            raise ValueError(f"kv_lanes: sequence {seq} outside the plan's {max(1, self.n_seqs)}")
        cache[seq] = (capi.KvLaneC * per)(*arr[seq * per:(seq + 1) * per])
        return cache[seq]

    def quant_bytes(self):
        n = C.c_uint64()
        b = self.lib.zh_model_quant_bytes(self.ptr, C.byref(n))
        return int(b), int(n.value)


class BatchModel(Model):
    """Synthetic weights + the BATCHED decode program (`build_batch_decode_program`): one step advances `n_seqs` independent
    sequences, each with its own KV slab, position and token. kv_quant_block=32: every sequence owns int8 KV caches instead of a
    slab (the builder's parameter; a cfg whose own kv_quant_block != 0 stays refused). tokens_per_seq=Ts in 2..16: every sequence
    owns Ts consecutive columns per step (column b * Ts + j is token j of sequence b): the plan of a batched verify step
    (BatchSession.resident_decode_batch_speculative). ValueError with the builder's text for what it refuses."""

    def __init__(self, cfg: Config, n_seqs: int, weight_kind: int = Q4_0, fused_elementwise: bool = True,
                 include_dead_f32: bool = False, threads: int = 8, like: Model = None, kv_quant_block: int = 0, tokens_per_seq: int = 1):
        """`like`: build the batched program over that model's weights (shared, not generated again; cfg / weight_kind come from it)."""
        self.lib = load_host()
        self.cfg = like.cfg if like else cfg
        self.n_seqs, self.tokens_per_seq = n_seqs, tokens_per_seq
        self.token_len = n_seqs * tokens_per_seq
        self.kv_quant_block = kv_quant_block
        err = C.create_string_buffer(256)
        if like:
            self.build_args = like.build_args
            self.ptr = self.lib.zh_model_create_batch_like_ts(like.ptr, int(like.build_args[1]), int(like.build_args[2]), n_seqs, kv_quant_block,
                                                              tokens_per_seq, err, len(err))
        else:
            self.build_args = (weight_kind, fused_elementwise, include_dead_f32, threads)
            self.ptr = self.lib.zh_model_create_batch_ts(C.byref(cfg), weight_kind, int(fused_elementwise), int(include_dead_f32), threads,
                                                         n_seqs, kv_quant_block, tokens_per_seq, err, len(err))
        if not self.ptr:
            raise ValueError(err.value.decode())

    def patch_batch(self, tokens, positions) -> None:
        t, p = np.ascontiguousarray(tokens, dtype=np.uint32), np.ascontiguousarray(positions, dtype=np.uint32)
        assert t.size == self.n_seqs * self.tokens_per_seq and p.size == self.n_seqs
        self.lib.zh_model_patch_batch(self.ptr, t.ctypes.data, p.ctypes.data)

    def dyn_sequences(self):
        """(op indices, sequence of each): every op with a position-dependent field (zgml_hip_program_set_sequences)."""
        n = self.lib.zh_model_dyn_sequences(self.ptr, None, None, 0)
        idx, seq = (C.c_uint32 * max(1, n))(), (C.c_uint32 * max(1, n))()
        self.lib.zh_model_dyn_sequences(self.ptr, idx, seq, n)
        return np.array(idx[:n], np.uint32), np.array(seq[:n], np.uint32)

    def kv_slab_elems(self) -> int:
        """f32 elements of one sequence's slab of a K or V buffer (= the single-sequence plan's whole buffer)."""
        return self.cfg.d_head * self.cfg.max_seq_len * self.cfg.n_kv_heads


def _kv_shift(session, lanes, keep: int, discard: int, n_filled: int) -> int:
    """zgml_hip_kv_shift over `lanes` of the session's program -> the new position. The lane order is (layer, kv head, K | V)
    with K | V innermost (DecodeProgram::kv_lanes), so every even lane is a K lane: those are the ones whose moved columns are
    turned back. The rows are the first half of row `discard` of the model's own RoPE tables."""
    cfg = session.model.cfg
    is_hip = capi.HIP_LIB_PATH.exists() and session.fns.compile_program == _fn_addr(capi.load_hip(), "zgml_hip_compile_program")
    if not is_hip:
        raise RuntimeError("kv_shift: a HIP session is needed")
    keep, discard, n_filled = int(keep), int(discard), int(n_filled)
    if keep < 0 or discard < 0 or keep + discard > n_filled or n_filled > cfg.max_seq_len:
        raise ValueError(f"kv_shift: keep {keep} + discard {discard} <= n_filled {n_filled} <= max_seq_len {cfg.max_seq_len} must hold")
    if discard == 0 or keep + discard == n_filled:
        return n_filled - discard  # (nothing moves)
    hd = cfg.d_head // 2
    cos, sin = session.model.rope_tables()
    c, s = np.ascontiguousarray(cos[discard, :hd], np.float32), np.ascontiguousarray(sin[discard, :hd], np.float32)
    rotate = (C.c_uint8 * len(lanes))(*[1 - i % 2 for i in range(len(lanes))])
    f32p = C.POINTER(C.c_float)
    hip = capi.load_hip()
    if hip.zgml_hip_kv_shift(session.fns.ctx, session.handle, lanes, rotate, len(lanes), keep, discard, n_filled, c.ctypes.data_as(f32p),
                             s.ctypes.data_as(f32p)) != 0:
        raise RuntimeError((hip.zgml_hip_last_error(session.fns.ctx) or b"").decode())
    return n_filled - discard


def _is_hip(session) -> bool:
    return capi.HIP_LIB_PATH.exists() and session.fns.compile_program == _fn_addr(capi.load_hip(), "zgml_hip_compile_program")


def _kv_park(session, lanes, n_cols: int, col: int, int8: bool) -> np.ndarray:
    """zgml_hip_kv_park over `lanes` of the session's program -> the blob (uint8; zgml_amd/csrc/kv_park.h states its layout)"""
    if not _is_hip(session):
        raise RuntimeError("kv_park: a HIP session is needed")
    n_cols, col, flags = int(n_cols), int(col), capi.KV_PARK_INT8 if int8 else 0
    if n_cols < 0 or col < 0:
        raise ValueError(f"kv_park: n_cols {n_cols} and col {col} must not be negative")
    hip = capi.load_hip()
    size = hip.zgml_hip_kv_park_bytes(lanes, len(lanes), n_cols, flags)
    blob = np.zeros(size, np.uint8)  # (size 0: a lane table the call refuses — it says why)
    if hip.zgml_hip_kv_park(session.fns.ctx, session.handle, lanes, len(lanes), col, n_cols, flags, blob.ctypes.data, size) != 0:
        raise RuntimeError((hip.zgml_hip_last_error(session.fns.ctx) or b"").decode())
    return blob


def _kv_resume(session, lanes, blob, col: int) -> None:
    if not _is_hip(session):
        raise RuntimeError("kv_resume: a HIP session is needed")
    if int(col) < 0:
        raise ValueError(f"kv_resume: col {col} must not be negative")
    blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, np.uint8)
    hip = capi.load_hip()
    if hip.zgml_hip_kv_resume(session.fns.ctx, session.handle, lanes, len(lanes), int(col), blob.ctypes.data, blob.size) != 0:
        raise RuntimeError((hip.zgml_hip_last_error(session.fns.ctx) or b"").decode())


class BatchSession:
    """Batched decode: `step` advances `n_seqs` sequences by one token each through the vtable (refresh + execute). `model` is a
    BatchModel of `n_seqs` sequences, or any other Model: the session then builds the batched program over that model's weights
    (shared, so the model must outlive the session). On the HIP backend the program is compiled with
    ZGML_HIP_OPT_SMALL_M_MATVEC on (`small_m_matvec=False`: the tile kernels; an int: the option's value, e.g. 8 = the row kernel up
    to its widest form) and its sequences are declared; the oracle
    takes the same program unchanged. kv_quant_block, tokens_per_seq: for the batched twin the session builds itself (a BatchModel
    carries its own)."""

    def __init__(self, model: Model, fns: BackendFns, n_seqs: int, small_m_matvec=True, kv_quant_block: int = 0, tokens_per_seq: int = 1):
        self.lib, self.fns, self.n_seqs = model.lib, fns, n_seqs
        self._own_model = not (isinstance(model, BatchModel) and model.n_seqs == n_seqs)
        self.model = BatchModel(model.cfg, n_seqs, like=model, kv_quant_block=kv_quant_block, tokens_per_seq=tokens_per_seq) if self._own_model else model
        self.tokens_per_seq = self.model.tokens_per_seq
        self.is_hip = capi.HIP_LIB_PATH.exists() and fns.compile_program == _fn_addr(capi.load_hip(), "zgml_hip_compile_program")
        hip = capi.load_hip() if self.is_hip else None
        if self.is_hip:  # (read at compile_program; other programs of the context keep the default)
            hip.zgml_hip_set_option(fns.ctx, capi.OPT_SMALL_M_MATVEC, int(small_m_matvec))
        try:
            self.ptr = self.lib.zh_session_create(self.model.ptr, C.byref(fns))
        finally:
            if self.is_hip:
                hip.zgml_hip_set_option(fns.ctx, capi.OPT_SMALL_M_MATVEC, 0)
        if not self.ptr:
            raise RuntimeError("compile_program failed")
        if self.is_hip:
            idx, seq = self.model.dyn_sequences()
            rc = hip.zgml_hip_program_set_sequences(fns.ctx, self.handle, n_seqs, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    seq.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size)
            if rc != 0:
                raise RuntimeError("set_sequences: " + (hip.zgml_hip_last_error(fns.ctx) or b"").decode())

    @property
    def handle(self):
        return self.lib.zh_session_handle(self.ptr)

    def use_dynamic_refresh(self, on: bool = True) -> None:
        """Per step hand over (slice_pos[B], seq_kv[B]) through zgml_hip_refresh_dynamic_batch instead of the whole op list."""
        self.lib.zh_session_set_refresh_dynamic_batch(self.ptr, _fn_addr(capi.load_hip(), "zgml_hip_refresh_dynamic_batch") if on else None)

    def step(self, tokens, positions):
        """-> (next_tokens[B], logits[B, vocab]); a tokens_per_seq = Ts plan takes B * Ts tokens (sequence-major) and B positions —
        sequence b runs its Ts tokens at positions[b] .. positions[b] + Ts - 1 — and returns B * Ts rows"""
        t, p = np.ascontiguousarray(tokens, dtype=np.uint32).ravel(), np.ascontiguousarray(positions, dtype=np.uint32)
        rows = self.n_seqs * self.tokens_per_seq
        assert t.size == rows and p.size == self.n_seqs
        logits = np.zeros((rows, self.model.cfg.vocab_size), np.float32)
        nxt = np.zeros(rows, np.int64)
        if self.lib.zh_session_step_batch(self.ptr, t.ctypes.data, p.ctypes.data, logits.ctypes.data, nxt.ctypes.data) != 0:
            raise ValueError("step: token or position out of range")
        return nxt, logits

    # ── KV admission (HIP backend only; include/zgml_hip.h zgml_hip_kv_move) ──
    def _kv_move(self, dst_lanes, src_handle, src_lanes, src_col, dst_col, n_cols) -> None:
        if not self.is_hip:
            raise RuntimeError("kv_move: a HIP session is needed")
        if len(dst_lanes) != len(src_lanes):
            raise ValueError(f"kv_move: {len(src_lanes)} source lanes for {len(dst_lanes)} destination lanes (plans of different configs)")
        hip = capi.load_hip()
        if hip.zgml_hip_kv_move(self.fns.ctx, self.handle, dst_lanes, src_handle, src_lanes, len(dst_lanes), src_col, dst_col, n_cols) != 0:
            raise RuntimeError("kv_move: " + (hip.zgml_hip_last_error(self.fns.ctx) or b"").decode())

    def admit(self, seq: int, src_session, n_cols: int, src_seq: int = 0) -> None:
        """Hand sequence `seq` the first n_cols KV columns of every cache of `src_session` (a Session over a decode or T-token plan
        of the same config on the same context, or a BatchSession and its sequence `src_seq`), in one launch on the context stream:
        copied, or quantised when this plan's caches are int8 and the source's f32."""
        self._kv_move(self.model.kv_lanes(seq), src_session.handle, src_session.model.kv_lanes(src_seq), 0, 0, n_cols)

    def fork(self, src_seq: int, dst_seq: int, n_cols: int) -> None:
        """Sequence dst_seq takes the first n_cols KV columns of sequence src_seq (n completions of one prompt)."""
        if src_seq == dst_seq:
            raise ValueError("fork: source and destination are the same sequence")
        self._kv_move(self.model.kv_lanes(dst_seq), self.handle, self.model.kv_lanes(src_seq), 0, 0, n_cols)

    def shift(self, seq: int, keep: int, discard: int, n_filled: int) -> int:
        """Context shift of sequence `seq` alone (Session.shift; include/zgml_hip.h zgml_hip_kv_shift): of its n_filled columns the
        first `keep` stay, the next `discard` are dropped, the rest move down with their keys turned back -> the sequence's new
        position n_filled - discard. The other sequences' caches are not touched. The caller drops the same tokens from whatever
        it keeps per sequence (`history` of the speculative loops, the penalties' window) and shifts a batched draft session's
        sequence too; an attached constraint needs nothing."""
        return _kv_shift(self, self.model.kv_lanes(seq), keep, discard, n_filled)

    def park(self, seq: int, n_cols: int, col: int = 0, int8: bool = False) -> np.ndarray:
        """KV columns [col, col + n_cols) of sequence `seq` -> a host blob (Session.park: the same call over this slot's lanes).
        The slot is free for another sequence afterwards (preemption); the other sequences' caches are not touched. What the
        caller keeps beside the blob, per sequence: its token history, the penalties' window, the constraint's state
        (constraint_state) and its position."""
        return _kv_park(self, self.model.kv_lanes(seq), n_cols, col, int8)

    def resume(self, seq: int, blob, col: int = 0) -> None:
        """The blob's columns -> columns [col, col + n) of sequence `seq` (Session.resume): any slot of any batched plan of the
        blob's model, f32 or int8, on any context — a prompt parked once can be resumed into many slots. Stream-ordered: the next
        step or resident loop sees the columns. The caller puts back what it kept beside the blob (history, penalty window,
        set_constraint with the saved state) and decodes on at the saved position."""
        _kv_resume(self, self.model.kv_lanes(seq), blob, col)

    # ── device-resident loop (HIP backend only; include/zgml_hip.h zgml_hip_resident_decode_batch) ──
    def resident_setup(self, backend) -> None:
        Session.resident_setup(self, backend)

    def set_constraint(self, constraint, state: int = 0, seq: int = 0) -> None:
        Session.set_constraint(self, constraint, state, seq)

    def constraint_state(self, seq: int = 0) -> int:
        return Session.constraint_state(self, seq)

    def resident_decode_batch(self, first_tokens, start_pos, n_steps) -> np.ndarray:
        """-> tokens[B, max(n_steps)]; row b holds n_steps[b] tokens, then -1."""
        u32p = C.POINTER(C.c_uint32)
        t, p = np.ascontiguousarray(first_tokens, dtype=np.uint32), np.ascontiguousarray(start_pos, dtype=np.uint32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_steps, dtype=np.uint32), (self.n_seqs,)))
        assert t.size == self.n_seqs and p.size == self.n_seqs
        max_steps = int(n.max()) if n.size else 0
        toks = np.full((self.n_seqs, max(1, max_steps)), -1, np.int64)
        rc = capi.load_hip().zgml_hip_resident_decode_batch(self._backend.ctx, self.handle, t.ctypes.data_as(u32p), p.ctypes.data_as(u32p),
                                                            n.ctypes.data_as(u32p), max_steps, toks.ctypes.data)
        if rc != 0:
            raise RuntimeError("resident_decode_batch: " + self._backend.last_error())
        return toks[:, :max_steps]

    def resident_decode_batch_speculative(self, first_tokens, start_pos, n_tokens, histories=None, drafts=None, ngram: int = 2):
        """Greedy-exact speculative decode of every sequence on a tokens_per_seq >= 2 plan (include/zgml_hip.h:
        zgml_hip_resident_decode_batch_speculative) -> (tokens[B, max(n_tokens)], [{"steps", "drafted", "accepted"}] per sequence);
        row b holds n_tokens[b] tokens, then -1. histories / drafts: None, or one entry per sequence as `history` / `drafts` of
        Session.resident_decode_speculative (an entry None: no history / the n-gram lookup)."""
        u32p = C.POINTER(C.c_uint32)
        B = self.n_seqs
        t, p = np.ascontiguousarray(first_tokens, dtype=np.uint32), np.ascontiguousarray(start_pos, dtype=np.uint32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_tokens, dtype=np.uint32), (B,)))
        assert t.size == B and p.size == B
        histories = [None] * B if histories is None else list(histories)
        drafts = [None] * B if drafts is None else list(drafts)
        assert len(histories) == B and len(drafts) == B
        opts, keep = (capi.SpecDecodeC * B)(), []
        for b in range(B):
            opts[b], arrays = Session._spec_opt(histories[b], drafts[b], ngram)
            keep.append(arrays)
        max_tokens = int(n.max()) if n.size else 0
        toks = np.full((B, max(1, max_tokens)), -1, np.int64)
        stats = (capi.SpecStatsC * B)()
        rc = capi.load_hip().zgml_hip_resident_decode_batch_speculative(self._backend.ctx, self.handle, t.ctypes.data_as(u32p), p.ctypes.data_as(u32p),
                                                                        n.ctypes.data_as(u32p), max_tokens, opts, toks.ctypes.data, stats)
        del keep
        if rc != 0:
            raise RuntimeError("resident_decode_batch_speculative: " + self._backend.last_error())
        return toks[:, :max_tokens], [{"steps": st.steps, "drafted": st.drafted, "accepted": st.accepted} for st in stats]

    def resident_decode_batch_speculative_sampled(self, first_tokens, start_pos, n_tokens, samplings, histories=None, drafts=None, ngram: int = 2,
                                                  logprobs=None):
        """Sampled speculative decode of every sequence on a tokens_per_seq >= 2 plan (include/zgml_hip.h:
        zgml_hip_resident_decode_batch_speculative_sampled): `samplings` is one capi.SamplingC per sequence, histories / drafts as
        in resident_decode_batch_speculative. -> (tokens[B, max(n_tokens)], n_produced[B], [{"steps", "drafted", "accepted"}] per
        sequence); row b holds n_produced[b] tokens — up to and including a stop token —, then -1. logprobs: True, or one flag per
        sequence: float32[B, max(n_tokens)] is appended, row b the log-probabilities of sequence b's tokens — NaN behind them, and
        all through a row whose flag is off."""
        return self._batch_speculative_sampled("resident_decode_batch_speculative_sampled", first_tokens, start_pos, n_tokens, samplings, histories, drafts,
                                               ngram, logprobs)

    def _batch_speculative_sampled(self, entry, first_tokens, start_pos, n_tokens, samplings, histories, drafts, ngram, logprobs):
        """the sampled and the constrained batched speculative call: one signature in the library, one marshalling here"""
        u32p = C.POINTER(C.c_uint32)
        B = self.n_seqs
        t, p = np.ascontiguousarray(first_tokens, dtype=np.uint32), np.ascontiguousarray(start_pos, dtype=np.uint32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_tokens, dtype=np.uint32), (B,)))
        assert t.size == B and p.size == B and len(samplings) == B
        histories = [None] * B if histories is None else list(histories)
        drafts = [None] * B if drafts is None else list(drafts)
        assert len(histories) == B and len(drafts) == B
        opts, keep = (capi.SpecDecodeC * B)(), []
        for b in range(B):
            opts[b], arrays = Session._spec_opt(histories[b], drafts[b], ngram)
            keep.append(arrays)
        sp = (capi.SamplingC * B)(*samplings)
        flags = [bool(logprobs)] * B if logprobs is None or isinstance(logprobs, bool) else [bool(x) for x in logprobs]
        assert len(flags) == B
        for b in range(B):
            if flags[b]:
                sp[b].logprobs = 1
        max_tokens = int(n.max()) if n.size else 0
        toks = np.full((B, max(1, max_tokens)), -1, np.int64)
        produced = np.zeros(B, np.uint32)
        stats = (capi.SpecStatsC * B)()
        rc = getattr(capi.load_hip(), "zgml_hip_" + entry)(
            self._backend.ctx, self.handle, t.ctypes.data_as(u32p), p.ctypes.data_as(u32p), n.ctypes.data_as(u32p), max_tokens, opts, sp, toks.ctypes.data,
            produced.ctypes.data_as(u32p), stats)
        del keep
        if rc != 0:
            raise RuntimeError(entry + ": " + self._backend.last_error())
        out = (toks[:, :max_tokens], produced, [{"steps": st.steps, "drafted": st.drafted, "accepted": st.accepted} for st in stats])
        if logprobs is None:
            return out
        asked = any(bool(sp[b].logprobs) for b in range(B))
        lps = capi.logprobs_result(self._backend.ctx, (B, max_tokens)) if asked and max_tokens else np.full((B, max_tokens), np.nan, np.float32)
        return out + (lps,)

    def resident_decode_batch_speculative_constrained(self, first_tokens, start_pos, n_tokens, samplings, histories=None, drafts=None, ngram: int = 2,
                                                      logprobs=None):
        """Constrained speculative decode of every sequence on a tokens_per_seq >= 2 plan (include/zgml_hip.h:
        zgml_hip_resident_decode_batch_speculative_constrained): resident_decode_batch_speculative_sampled whose sequences walk the
        automata attached through set_constraint(constraint, state, seq) — each its own, sequences with and without one side by
        side. Arguments and results are the sampled call's; a sequence whose state allows no token ends early, as behind a stop
        token (n_produced[b] counts what came out; constraint_state(b) reads the state it reached)."""
        return self._batch_speculative_sampled("resident_decode_batch_speculative_constrained", first_tokens, start_pos, n_tokens, samplings, histories, drafts,
                                               ngram, logprobs)

    def resident_decode_batch_speculative_model(self, draft_session: "BatchSession", first_tokens, start_pos, n_tokens, samplings=None, histories=None,
                                                logprobs=None):
        """zgml_hip_resident_decode_batch_speculative_model: every sequence of this session's tokens_per_seq = T >= 2 plan verifies
        what `draft_session`'s batched one-column plan (same backend, n_seqs and vocabulary, its own resident_setup) drafts
        greedily for it, T - 1 tokens per step, all on the device. Both sessions' caches must hold every sequence's positions <
        start_pos[b]; afterwards both hold those < start_pos[b] + its produced count. samplings=None: the greedy verify step; else
        one capi.SamplingC per sequence, as in resident_decode_batch_speculative_sampled. histories: None, or per sequence None /
        the tokens at positions 0..start_pos[b]-1. -> (tokens[B, max(n_tokens)], n_produced[B], [{"steps", "drafted",
        "accepted"}] per sequence); logprobs (True, or one flag per sequence; needs samplings): float32[B, max(n_tokens)] is
        appended, as there."""
        u32p = C.POINTER(C.c_uint32)
        B = self.n_seqs
        t, p = np.ascontiguousarray(first_tokens, dtype=np.uint32), np.ascontiguousarray(start_pos, dtype=np.uint32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_tokens, dtype=np.uint32), (B,)))
        assert t.size == B and p.size == B and (samplings is None or len(samplings) == B)
        if samplings is None and logprobs:
            raise ValueError("resident_decode_batch_speculative_model: logprobs need the sampling parameter sets")
        hists = [np.ascontiguousarray([] if h is None else h, dtype=np.uint32) for h in ([None] * B if histories is None else histories)]
        assert len(hists) == B
        hist_ptrs = (u32p * B)(*[h.ctypes.data_as(u32p) if h.size else None for h in hists])
        n_hist = np.array([h.size for h in hists], np.uint32)
        sp = None
        if samplings is not None:
            sp = (capi.SamplingC * B)(*samplings)
            flags = [bool(logprobs)] * B if logprobs is None or isinstance(logprobs, bool) else [bool(x) for x in logprobs]
            assert len(flags) == B
            for b in range(B):
                if flags[b]:
                    sp[b].logprobs = 1
        max_tokens = int(n.max()) if n.size else 0
        toks = np.full((B, max(1, max_tokens)), -1, np.int64)
        produced = np.zeros(B, np.uint32)
        stats = (capi.SpecStatsC * B)()
        rc = capi.load_hip().zgml_hip_resident_decode_batch_speculative_model(
            self._backend.ctx, self.handle, draft_session.handle if draft_session is not None else None, t.ctypes.data_as(u32p), p.ctypes.data_as(u32p),
            n.ctypes.data_as(u32p), max_tokens, hist_ptrs, n_hist.ctypes.data_as(u32p), sp, toks.ctypes.data, produced.ctypes.data_as(u32p), stats)
        if rc != 0:
            raise RuntimeError("resident_decode_batch_speculative_model: " + self._backend.last_error())
        out = (toks[:, :max_tokens], produced, [{"steps": st.steps, "drafted": st.drafted, "accepted": st.accepted} for st in stats])
        if logprobs is None:
            return out
        asked = any(bool(sp[b].logprobs) for b in range(B))
        lps = capi.logprobs_result(self._backend.ctx, (B, max_tokens)) if asked and max_tokens else np.full((B, max_tokens), np.nan, np.float32)
        return out + (lps,)

    def resident_decode_batch_sampled(self, first_tokens, start_pos, n_steps, samplings, logprobs=None, top_logprobs=None):
        """zgml_hip_resident_decode_batch_sampled: `samplings` is one capi.SamplingC per sequence.
        -> (tokens[B, max(n_steps)], n_produced[B]); row b holds n_produced[b] tokens, then -1. logprobs: True, or one flag per
        sequence: -> (tokens, n_produced, float32[B, max(n_steps)]), row b the log-probabilities of sequence b's tokens — NaN
        behind them, and all through a row whose flag is off. top_logprobs: an int, or one per sequence (a count > 0 sets the
        sequence's flag too): (int64[B, max(n_steps), width], float32[...]) is appended, the alternatives of every token — width
        the largest effective count, -1 / NaN as padding and behind the tokens."""
        u32p = C.POINTER(C.c_uint32)
        t, p = np.ascontiguousarray(first_tokens, dtype=np.uint32), np.ascontiguousarray(start_pos, dtype=np.uint32)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_steps, dtype=np.uint32), (self.n_seqs,)))
        assert t.size == self.n_seqs and p.size == self.n_seqs and len(samplings) == self.n_seqs
        sp = (capi.SamplingC * self.n_seqs)(*samplings)
        max_steps = int(n.max()) if n.size else 0
        toks = np.full((self.n_seqs, max(1, max_steps)), -1, np.int64)
        produced = np.zeros(self.n_seqs, np.uint32)
        flags = [bool(logprobs)] * self.n_seqs if logprobs is None or isinstance(logprobs, bool) else [bool(x) for x in logprobs]
        tops = [0] * self.n_seqs if top_logprobs is None else [int(top_logprobs)] * self.n_seqs if np.isscalar(top_logprobs) else [int(x) for x in top_logprobs]
        assert len(tops) == self.n_seqs
        flags = [f or a > 0 for f, a in zip(flags, tops)]
        for b in range(self.n_seqs):
            if flags[b]:
                sp[b].logprobs = 1
            if top_logprobs is not None:
                sp[b].top_logprobs = tops[b]
        rc = capi.load_hip().zgml_hip_resident_decode_batch_sampled(self._backend.ctx, self.handle, t.ctypes.data_as(u32p), p.ctypes.data_as(u32p),
                                                                    n.ctypes.data_as(u32p), max_steps, sp, toks.ctypes.data, produced.ctypes.data_as(u32p))
        if rc != 0:
            raise RuntimeError("resident_decode_batch_sampled: " + self._backend.last_error())
        if logprobs is None and top_logprobs is None:
            return toks[:, :max_steps], produced
        lps = capi.logprobs_result(self._backend.ctx, (self.n_seqs, max_steps)) if any(flags) and max_steps else np.full((self.n_seqs, max_steps), np.nan, np.float32)
        if top_logprobs is None:
            return toks[:, :max_steps], produced, lps
        if any(tops) and max_steps:
            alts = capi.top_logprobs_result(self._backend.ctx, (self.n_seqs, max_steps))
        else:
            alts = np.full((self.n_seqs, max_steps, 0), -1, np.int64), np.full((self.n_seqs, max_steps, 0), np.nan, np.float32)
        return toks[:, :max_steps], produced, lps, alts

    def close(self):
        if self.ptr:
            self.lib.zh_session_free(self.ptr)
            self.ptr = None
        if self._own_model:
            self.model.close()


class Session:
    """`LlamaDeviceSession`: compile once, then doStep per token through the vtable."""

    def __init__(self, model: Model, fns: BackendFns):
        self.model, self.lib, self.fns = model, model.lib, fns
        self.ptr = self.lib.zh_session_create(model.ptr, C.byref(fns))
        if not self.ptr:
            raise RuntimeError("compile_program failed")

    @property
    def handle(self):
        return self.lib.zh_session_handle(self.ptr)

    def use_dynamic_refresh(self, on: bool = True) -> None:
        """The adapter's per-token refresh (zig/backend_hip.zig: refreshProgram): (slice_pos, seq_kv) through
        zgml_hip_refresh_dynamic instead of the whole op list through zgml_hip_refresh_program. HIP sessions only."""
        self.lib.zh_session_set_refresh_dynamic(self.ptr, _fn_addr(capi.load_hip(), "zgml_hip_refresh_dynamic") if on else None)

    def pin_outputs(self, backend, on: bool = True) -> None:
        """The adapter's promise that the session's logits buffer outlives the program (zgml_hip_program_pin_outputs): the step's
        last kernel then writes the logits straight into it. HIP sessions only."""
        capi.load_hip().zgml_hip_program_pin_outputs(backend.ctx, self.handle, 1 if on else 0)

    def step(self, token: int, pos: int, want_logits: bool = True):
        logits = np.zeros(self.model.cfg.vocab_size, np.float32) if want_logits else None
        nxt = self.lib.zh_session_step(self.ptr, token, pos, logits.ctypes.data if want_logits else None)
        return int(nxt), logits

    def prefill(self, tokens, pos: int, want_logits: bool = True):
        """One execution of a token_len = N plan: returns (greedy token, logits of the last position)."""
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        assert toks.size == self.model.token_len
        logits = np.zeros(self.model.cfg.vocab_size, np.float32) if want_logits else None
        nxt = self.lib.zh_session_prefill(self.ptr, toks.ctypes.data, pos, logits.ctypes.data if want_logits else None)
        return int(nxt), logits

    def decode(self, first_token: int, start_pos: int, n_steps: int):
        toks = np.zeros(n_steps, np.int64)
        secs = self.lib.zh_session_decode(self.ptr, first_token, start_pos, n_steps, toks.ctypes.data)
        return toks, secs

    def shift(self, keep: int, discard: int, n_filled: int) -> int:
        """Context shift (HIP sessions only, like BatchSession.admit / fork; include/zgml_hip.h zgml_hip_kv_shift): with n_filled
        KV columns in use, keep the first `keep` (BOS / system prompt), drop the next `discard`, move the rest down and turn every
        moved key back by `discard` positions of RoPE — one stream-ordered launch, no forward pass -> the new position
        n_filled - discard, where step / resident_decode* go on (generation past max_seq_len). What the caller owns: drop tokens
        [keep, keep + discard) from the `history` it hands the speculative loops (and from a penalty window it tracks), and shift
        a draft model's session with the same arguments (a draft pair is shifted by shifting both sessions). Constraint state
        needs nothing: it depends on tokens, not positions. int8 caches are requantised on every shift (truncation shrinks the
        keys a little each time): shift rarely and by much — at half the window a column is requantised at most twice. The
        shifted cache is not a re-prefilled one: kept columns still carry the attention of the dropped tokens (llama.cpp's
        semantics)."""
        return _kv_shift(self, self.model.kv_lanes(), keep, discard, n_filled)

    def park(self, n_cols: int, col: int = 0, int8: bool = False) -> np.ndarray:
        """KV columns [col, col + n_cols) of every cache -> a host blob (uint8 array; HIP sessions only; include/zgml_hip.h
        zgml_hip_kv_park): one pack launch and one device-to-host copy, complete on return. The blob outlives the session, the
        model's plan and the backend: keep it as a prompt cache, to make room for a more urgent request, or across a restart
        (it is self-describing: zgml_amd/csrc/kv_park.h; writing it to a file is the caller's). int8=True stores f32 caches
        quantised with the cache's own column rule (0.28x the bytes at d_head 128); such a blob resumes into int8 plans only.
        What the caller still owns per sequence, because none of it lives in the caches: the token history, the penalties'
        window, the constraint's state and the position to decode on at."""
        return _kv_park(self, self.model.kv_lanes(), n_cols, col, int8)

    def resume(self, blob, col: int = 0) -> None:
        """The blob's columns -> columns [col, col + n) of every cache (zgml_hip_kv_resume): one host-to-device copy and one
        stream-ordered unpack launch; the blob may be dropped on return. f32 columns are quantised on the way into an int8 plan
        exactly as admission does; an int8 blob into an f32 plan is refused. `col` need not be the park's. History, penalty
        window, constraint state and position are put back by the caller."""
        _kv_resume(self, self.model.kv_lanes(), blob, col)

    # ── device-resident loop (HIP backend only; include/zgml_hip.h zgml_hip_resident_*) ──
    def resident_setup(self, backend) -> None:
        m, cfg = self.model, self.model.cfg
        hip = capi.load_hip()
        cos, sin = m.rope_tables()
        ropes = (C.c_uint16 * cfg.n_layers)(*[m.buf("rope", l) for l in range(cfg.n_layers)])
        d = capi.ResidentLlamaC()
        d.token_embed = m.token_embed().ctypes.data
        d.cos_table, d.sin_table = cos.ctypes.data, sin.ctypes.data
        d.vocab, d.d_model, d.max_seq, d.d_head = cfg.vocab_size, cfg.d_model, cfg.max_seq_len, cfg.d_head
        d.buf_token_input, d.buf_attn_mask, d.buf_logits = m.buf("token_input"), m.buf("attn_mask"), m.buf("logits")
        d.buf_rope, d.n_rope = C.cast(ropes, C.POINTER(C.c_uint16)), cfg.n_layers
        self._resident_keep = (ropes, cos, sin)
        if hip.zgml_hip_resident_setup(backend.ctx, self.handle, C.byref(d)) != 0:
            raise RuntimeError("resident_setup: " + backend.last_error())
        self._backend = backend

    def set_constraint(self, constraint, state: int = 0, seq: int = 0) -> None:
        """Attach a token automaton (Backend.constraint_create) to sequence `seq` at `state`, after resident_setup; None
        detaches. resident_decode_sampled / resident_decode_batch_sampled and Backend.sample then pick among the allowed tokens
        only, and the state advances on the device."""
        self._backend.set_constraint(self.handle, seq, constraint, state)

    def constraint_state(self, seq: int = 0) -> int:
        """the sequence's current state (-1: no constraint attached)"""
        return self._backend.constraint_state(self.handle, seq)

    def resident_decode(self, first_token: int, start_pos: int, n_steps: int) -> np.ndarray:
        toks = np.zeros(n_steps, np.int64)
        rc = capi.load_hip().zgml_hip_resident_decode(self._backend.ctx, self.handle, first_token, start_pos, n_steps,
                                                      toks.ctypes.data)
        if rc != 0:
            raise RuntimeError("resident_decode: " + self._backend.last_error())
        return toks

    def resident_decode_sampled(self, first_token: int, start_pos: int, n_steps: int, sampling: "capi.SamplingC", logprobs: bool = False, top_logprobs: int = 0):
        """zgml_hip_resident_decode_sampled -> (tokens[n_steps], n_produced): -1 behind a stop token. logprobs=True:
        -> (tokens, n_produced, float32[n_steps]): every token's log-probability, NaN behind a stop token. top_logprobs=a > 0:
        (int64[n_steps, min(a, 64, vocab)], float32[...]) is appended: every token's alternatives, -1 / NaN behind a stop token."""
        toks = np.full(max(1, n_steps), -1, np.int64)
        produced = C.c_uint32(0)
        if logprobs or top_logprobs:
            sampling = capi.with_logprobs(sampling, top=top_logprobs)
        rc = capi.load_hip().zgml_hip_resident_decode_sampled(self._backend.ctx, self.handle, first_token, start_pos, n_steps, C.byref(sampling),
                                                              toks.ctypes.data, C.byref(produced))
        if rc != 0:
            raise RuntimeError("resident_decode_sampled: " + self._backend.last_error())
        if not logprobs and not top_logprobs:
            return toks[:n_steps], int(produced.value)
        lps = capi.logprobs_result(self._backend.ctx, n_steps) if n_steps else np.zeros(0, np.float32)
        if not top_logprobs:
            return toks[:n_steps], int(produced.value), lps
        return toks[:n_steps], int(produced.value), lps, self._alternatives(n_steps)

    def _alternatives(self, entries: int):
        if entries:
            return capi.top_logprobs_result(self._backend.ctx, entries)
        return np.zeros((0, 0), np.int64), np.zeros((0, 0), np.float32)

    def resident_prefill(self, tokens, start_pos: int) -> int:
        """One chunk of a token_len = N plan with on-device embedding gather / mask / RoPE rows / argmax."""
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        nxt = int(capi.load_hip().zgml_hip_resident_prefill(self._backend.ctx, self.handle, toks.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                            toks.size, start_pos))
        if nxt < 0:
            raise RuntimeError("resident_prefill: " + self._backend.last_error())
        return nxt

    @staticmethod
    def _spec_opt(history, drafts, ngram: int):
        """-> (capi.SpecDecodeC, the arrays it points into: keep them alive over the call)"""
        u32p = C.POINTER(C.c_uint32)
        opt = capi.SpecDecodeC()
        hist = np.ascontiguousarray([] if history is None else history, dtype=np.uint32)
        dr = np.ascontiguousarray([] if drafts is None else drafts, dtype=np.uint32)
        opt.history, opt.n_history = (hist.ctypes.data_as(u32p) if hist.size else None), hist.size
        opt.mode, opt.ngram = (0 if drafts is None else 1), ngram
        opt.drafts, opt.n_drafts = (dr.ctypes.data_as(u32p) if dr.size else None), dr.size
        return opt, (hist, dr)

    def resident_decode_speculative(self, first_token: int, start_pos: int, n_tokens: int, history=None, drafts=None, ngram: int = 2):
        """Greedy-exact speculative decode on a token_len = T >= 2 plan (include/zgml_hip.h: zgml_hip_resident_decode_speculative):
        -> (tokens[n_tokens], {"steps", "drafted", "accepted"}). `history`: the tokens at positions 0..start_pos-1 (None: the n-gram
        lookup sees only this call's tokens). `drafts`: guesses for the tokens at positions start_pos+1.. (provided mode); None:
        n-gram lookup with suffixes of up to `ngram` tokens."""
        opt, keep = self._spec_opt(history, drafts, ngram)
        toks = np.zeros(n_tokens, np.int64)
        stats = capi.SpecStatsC()
        rc = capi.load_hip().zgml_hip_resident_decode_speculative(self._backend.ctx, self.handle, first_token, start_pos, n_tokens, C.byref(opt),
                                                                   toks.ctypes.data, C.byref(stats))
        del keep
        if rc != 0:
            raise RuntimeError("resident_decode_speculative: " + self._backend.last_error())
        return toks, {"steps": stats.steps, "drafted": stats.drafted, "accepted": stats.accepted}

    def resident_decode_speculative_constrained(self, first_token: int, start_pos: int, n_tokens: int, sampling: "capi.SamplingC", history=None,
                                                drafts=None, ngram: int = 2, logprobs: bool = False, top_logprobs: int = 0):
        """zgml_hip_resident_decode_speculative_constrained: resident_decode_speculative_sampled whose verify rows walk the automaton
        attached to the sequence (set_constraint) — forced tokens are drafted for free, every pick is masked by its row's state and
        the device state advances over the emitted tokens. The same arguments and the same result; n_produced is also short when a
        reached state allows no token. Without a constraint it is resident_decode_speculative_sampled."""
        return self.resident_decode_speculative_sampled(first_token, start_pos, n_tokens, sampling, history, drafts, ngram, logprobs, top_logprobs,
                                                        _entry="zgml_hip_resident_decode_speculative_constrained")

    def resident_decode_speculative_sampled(self, first_token: int, start_pos: int, n_tokens: int, sampling: "capi.SamplingC", history=None,
                                            drafts=None, ngram: int = 2, logprobs: bool = False, top_logprobs: int = 0,
                                            _entry: str = "zgml_hip_resident_decode_speculative_sampled"):
        """zgml_hip_resident_decode_speculative_sampled: the verify step's rows are sampled (seeded top-k / top-p) instead of
        arg-maxed -> (tokens[n_tokens], n_produced, {"steps", "drafted", "accepted"}): -1 behind a stop token. `history`, `drafts`
        and `ngram` as resident_decode_speculative. logprobs=True: float32[n_tokens] is appended to the result: every emitted
        token's log-probability, NaN behind a stop token. top_logprobs=a > 0: (int64[n_tokens, min(a, 64, vocab)], float32[...]) is
        appended too: every emitted token's alternatives under the row of the verify step that emitted it."""
        opt, keep = self._spec_opt(history, drafts, ngram)
        toks = np.full(max(1, n_tokens), -1, np.int64)
        if logprobs or top_logprobs:
            sampling = capi.with_logprobs(sampling, top=top_logprobs)
        stats, produced = capi.SpecStatsC(), C.c_uint32(0)
        rc = getattr(capi.load_hip(), _entry)(self._backend.ctx, self.handle, first_token, start_pos, n_tokens, C.byref(opt),
                                              C.byref(sampling), toks.ctypes.data, C.byref(produced), C.byref(stats))
        del keep
        if rc != 0:
            raise RuntimeError(_entry[len("zgml_hip_"):] + ": " + self._backend.last_error())
        st = {"steps": stats.steps, "drafted": stats.drafted, "accepted": stats.accepted}
        if not logprobs and not top_logprobs:
            return toks[:n_tokens], int(produced.value), st
        lps = capi.logprobs_result(self._backend.ctx, n_tokens) if n_tokens else np.zeros(0, np.float32)
        if not top_logprobs:
            return toks[:n_tokens], int(produced.value), st, lps
        return toks[:n_tokens], int(produced.value), st, lps, self._alternatives(n_tokens)

    def resident_decode_speculative_model_constrained(self, draft_session: "Session", first_token: int, start_pos: int, n_tokens: int,
                                                      sampling: "capi.SamplingC", history=None, logprobs: bool = False, top_logprobs: int = 0):
        """zgml_hip_resident_decode_speculative_model_constrained: resident_decode_speculative_model under the automaton attached to
        THIS session (set_constraint) — every draft is the draft model's first maximum over the tokens the walk's state allows, so
        forced tokens are drafted as they are and no verify row is spent on a forbidden one; the verify step is that of
        resident_decode_speculative_constrained. `sampling` is required (top_k = 1: greedy). The result is that of
        resident_decode_speculative_model with a sampling set; n_produced is also short when a reached state allows no token.
        Without a constraint it is resident_decode_speculative_model with `sampling`."""
        if sampling is None:
            raise ValueError("resident_decode_speculative_model_constrained: a sampling parameter set is required (top_k = 1 is the greedy form)")
        return self.resident_decode_speculative_model(draft_session, first_token, start_pos, n_tokens, sampling, history, logprobs, top_logprobs,
                                                      _entry="zgml_hip_resident_decode_speculative_model_constrained")

    def resident_decode_speculative_model(self, draft_session: "Session", first_token: int, start_pos: int, n_tokens: int, sampling=None, history=None,
                                          logprobs: bool = False, top_logprobs: int = 0, _entry: str = "zgml_hip_resident_decode_speculative_model"):
        """zgml_hip_resident_decode_speculative_model: this session's token_len = T >= 2 plan verifies what `draft_session`'s
        token_len = 1 plan (same backend, same vocabulary, its own resident_setup) drafts greedily, T - 1 tokens per step, all on
        the device. Both caches must hold the positions < start_pos; afterwards both hold those < start_pos + the produced count.
        sampling=None: the greedy verify step -> (tokens[n_tokens], {"steps", "drafted", "accepted"}). With a capi.SamplingC the
        result is that of resident_decode_speculative_sampled: (tokens, n_produced, stats), then the log-probabilities
        (logprobs=True) and the alternatives (top_logprobs > 0). `history`: the tokens at positions 0..start_pos-1 (the penalties'
        window reads them)."""
        u32p = C.POINTER(C.c_uint32)
        hist = np.ascontiguousarray([] if history is None else history, dtype=np.uint32)
        toks = np.full(max(1, n_tokens), -1, np.int64)
        if sampling is None and (logprobs or top_logprobs):
            raise ValueError("resident_decode_speculative_model: logprobs / top_logprobs need a sampling parameter set")
        if logprobs or top_logprobs:
            sampling = capi.with_logprobs(sampling, top=top_logprobs)
        stats, produced = capi.SpecStatsC(), C.c_uint32(0)
        rc = getattr(capi.load_hip(), _entry)(
            self._backend.ctx, self.handle, draft_session.handle if draft_session is not None else None, first_token, start_pos, n_tokens,
            hist.ctypes.data_as(u32p) if hist.size else None, hist.size, C.byref(sampling) if sampling is not None else None, toks.ctypes.data,
            C.byref(produced), C.byref(stats))
        if rc != 0:
            raise RuntimeError(_entry[len("zgml_hip_"):] + ": " + self._backend.last_error())
        st = {"steps": stats.steps, "drafted": stats.drafted, "accepted": stats.accepted}
        if sampling is None:
            return toks[:n_tokens], st
        if not logprobs and not top_logprobs:
            return toks[:n_tokens], int(produced.value), st
        lps = capi.logprobs_result(self._backend.ctx, n_tokens) if n_tokens else np.zeros(0, np.float32)
        if not top_logprobs:
            return toks[:n_tokens], int(produced.value), st, lps
        return toks[:n_tokens], int(produced.value), st, lps, self._alternatives(n_tokens)

    def close(self):
        if self.ptr:
            self.lib.zh_session_free(self.ptr)
            self.ptr = None
