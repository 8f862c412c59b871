// switches.h — every ZGML_* environment switch of libzgml_hip, declared once: the field, the environment name, the default and
// what it does (INTEGRATION.md section 9 has the longer story). Plain host C++ (nothing from HIP), so a test can compile it alone.
// sw() fills the table on its FIRST call (not at load), so a process may still set a variable after it has loaded the library
// and before it first uses it; after that a change is not seen. Rows built with trace(...) only look at the environment in the
// diagnostics build (-DZGML_TRACE); the product build always has their default.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace zgml {

// ── parse helpers, one per idiom; a null `name` (a trace-only row in the product build) counts as unset. env_int / env_long
// are atoi / atol ("0x10" is 0); the ..0 forms take base 0 ("0x10" is 16) ──
inline const char* env_text(const char* name) { return name ? getenv(name) : nullptr; }
inline int env_int(const char* name, int dflt) { const char* v = env_text(name); return v ? atoi(v) : dflt; }
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }
inline long env_long(const char* name, long dflt) { const char* v = env_text(name); return v ? atol(v) : dflt; }
inline long env_long0(const char* name, long dflt) { const char* v = env_text(name); return v ? strtol(v, nullptr, 0) : dflt; }
inline unsigned long env_ulong0(const char* name, unsigned long dflt) { const char* v = env_text(name); return v ? strtoul(v, nullptr, 0) : dflt; }
inline unsigned long long env_u64_0(const char* name, unsigned long long dflt) { const char* v = env_text(name); return v ? strtoull(v, nullptr, 0) : dflt; }
struct SetInt { bool set; int value; }; // "is it set at all" next to the integer value (0 when unset)
inline SetInt env_set_int(const char* name) { return SetInt{env_text(name) != nullptr, env_int(name, 0)}; }
#ifdef ZGML_TRACE // a switch that only exists in the diagnostics build
constexpr const char* trace(const char* name) { return name; }
#else
constexpr const char* trace(const char*) { return nullptr; }
#endif

struct Switches {
    // ── planner (plan.hip) ──
    bool hip_fuse_split = env_flag("ZGML_HIP_FUSE_SPLIT", true);                      // an M > 1 matmul takes its pre-laid-out A operand from the producing launch
    bool hip_fuse_qkv_attn = env_flag("ZGML_HIP_FUSE_QKV_ATTN", true);                // q / k / v projection + decode attention as one launch
    bool hip_fuse_qkv_attn_kon = env_flag("ZGML_HIP_FUSE_QKV_ATTN_KON", true);        // ... also for K-on-lanes models (K > 2048)
    int hip_fuse_kon_cap_eighths = env_int("ZGML_HIP_FUSE_KON_CAP_EIGHTHS", 8);       // share of the workgroup capacity that launch may fill
    bool hip_fuse_census = env_flag("ZGML_HIP_FUSE_CENSUS", true);                    // co-residency census of the fused K-on-lanes grid
    bool hip_ksplit_fuse_a = env_flag("ZGML_HIP_KSPLIT_FUSE_A", true);                // K-split layers: projection + attention as one launch
    bool hip_prenorm = env_flag("ZGML_HIP_PRENORM", true);                            // the residual epilogue prepares the next launch's rmsnorm
    bool hip_pair = env_flag("ZGML_HIP_PAIR", true);                                  // gate / up computed in pairs with the SiLU product stored by the launch
    bool hip_hoist_repeat = env_flag("ZGML_HIP_HOIST_REPEAT", true);                  // repeats of constant data leave the per-execution plan
    bool hip_attn_decode = env_flag("ZGML_HIP_ATTN_DECODE", true);                    // rope + cache store + attention of a decode step folded into one launch
    bool hip_attn_decode_kvq = env_flag("ZGML_HIP_ATTN_DECODE_KVQ", true);            // ... over quantised KV caches too
    bool hip_row_chain = env_flag("ZGML_HIP_ROW_CHAIN", true);                        // [add ->] rmsnorm [-> mul] on the same rows as one launch (M > 1)
    bool hip_elt_chain = env_flag("ZGML_HIP_ELT_CHAIN", true);                        // elementwise ops over the same elements as one launch
    int hip_attn_split = env_int("ZGML_HIP_ATTN_SPLIT", 16);                          // most key-range splits of a decode attention head (<= 1: never split)
    int hip_attn_split_min_keys = env_int("ZGML_HIP_ATTN_SPLIT_MIN_KEYS", -1);        // fewest keys per split (< 0: the caller's default; 0: never split)
    int hip_attn_split_wgs = env_int("ZGML_HIP_ATTN_SPLIT_WGS", 256);                 // workgroup budget that caps heads x splits
    bool hip_ks_trace = env_flag("ZGML_HIP_KS_TRACE", false);                         // stamp buffers for the K-split launches (the stamps exist in the diagnostics build)
    bool hip_attn_trace = env_flag("ZGML_HIP_ATTN_TRACE", false);                     // ... for the decode-attention launches
    bool hip_qmv_trace = env_flag("ZGML_HIP_QMV_TRACE", false);                       // ... for the mat-vec launches
    SetInt hip_debug_plan = env_set_int("ZGML_HIP_DEBUG_PLAN");                       // set (even to 0): print the plan summary; >= 2: per-launch times when profiling
    // ── runtime (runtime.hip, runtime_shard.hip) ──
    const char* hip_graph_dump = env_text("ZGML_HIP_GRAPH_DUMP");                     // directory for a .dot file of every instantiated graph
    unsigned hip_skip_kinds = (unsigned)env_ulong0(trace("ZGML_HIP_SKIP_KINDS"), 0);  // bitmask of launch kinds to drop (timing only: wrong results)
    const char* hip_skip_mod = env_text(trace("ZGML_HIP_SKIP_MOD"));                  // "<period>:<hex mask>": drop launch i >= 1 when bit (i-1) % period is set
    int hip_graph_split = env_int("ZGML_HIP_GRAPH_SPLIT", -1);                        // launches in the first of the token's two graphs (0: one graph; < 0: a sixth)
    bool hip_qmv_kon = env_flag("ZGML_HIP_QMV_KON", true);                            // mat-vec-only Q4_0 weights take the K-on-lanes layout
    int hip_qmv_kon_min_k = env_int("ZGML_HIP_QMV_KON_MIN_K", 2049);                  // ... from this K on
    bool hip_weight_arena = env_flag("ZGML_HIP_WEIGHT_ARENA", true);                  // a program's packed weights in two allocations, back to back
    uint64_t hip_nt_min_bytes = env_u64_0("ZGML_HIP_NT_MIN_BYTES", 192ull << 20);     // weight sets from this size on are streamed with non-temporal loads
    bool hip_io_graph = env_flag("ZGML_HIP_IO_GRAPH", true);                          // execute_program as one graph that reads / writes pinned host memory
    int hip_resident_tokens_per_graph = env_int("ZGML_HIP_RESIDENT_TOKENS_PER_GRAPH", 1); // tokens held by one graph of the resident loop
    int shard_peer_wait_ms = env_int("ZGML_SHARD_PEER_WAIT_MS", 5000);                // bound of a peer gather's wait (at least 1)
    bool shard_pair_argmax = env_flag("ZGML_SHARD_PAIR_ARGMAX", true);                // sharded greedy token from one (max, index) pair per rank
    bool shard_graph = env_flag("ZGML_SHARD_GRAPH", true);                            // a sharded step is captured into a graph
    // ── generic kernels (kernels_generic.hip, attention_tiles.hip) ──
    bool hip_elt_preload = env_flag("ZGML_HIP_ELT_PRELOAD", true);                    // elementwise chains load every step's second operand up front
    uint32_t hip_elt_vec4_min = (uint32_t)env_long("ZGML_HIP_ELT_VEC4_MIN", 1l << 20); // chain length from which a thread takes four elements
    int hip_row_split = env_int("ZGML_HIP_ROW_SPLIT", 0);                             // workgroups per row of a row chain (0: by the row count)
    int hip_attn_decode_block = env_int("ZGML_HIP_ATTN_DECODE_BLOCK", 0);             // 256 | 1024: workgroup size of the stand-alone decode attention (0: by d_head)
    bool hip_attn_rows = env_flag("ZGML_HIP_ATTN_ROWS", true);                        // dense prefill attention through the row / tile kernels
    int copy_variant = (int)env_long0("ZGML_COPY_VARIANT", 8 | 1 << 8 | 32 << 16);    // copy kernel: loads in flight | nt << 8 | blocks per CU << 16 (0: the plain loop)
    bool hip_attn_tiles = env_flag("ZGML_HIP_ATTN_TILES", true);                      // prefill attention on the f32-MFMA tile kernel
    int hip_attn_tiles_waves = env_int("ZGML_HIP_ATTN_TILES_WAVES", 0);               // its waves per workgroup (0: by the grid)
    // ── quantized mat-vec (qmatvec.hip) ──
    bool qmv_xdirect = env_flag("ZGML_QMV_XDIRECT", true);                            // x read straight from memory instead of staged in LDS
    bool qmv_xdirect_norm = env_flag("ZGML_QMV_XDIRECT_NORM", true);                  // ... also under an rmsnorm prologue
    int qmv_xdnorm_maxk = env_int("ZGML_QMV_XDNORM_MAXK", 2048);                      // ... up to this K
    bool qmv_contig = env_flag("ZGML_QMV_CONTIG", true);                              // parts back to back in the arena are found without the argument block
    bool qmv_epi_silu = env_flag("ZGML_QMV_EPI_SILU", true);                          // the SiLU chain as a compiled epilogue (and the pair launch built on it)
    int qmv_waves = env_int("ZGML_QMV_WAVES", 0);                                     // waves per workgroup of the n-on-lanes mat-vec (0: by K)
    int qmv_waves_smallk = env_int("ZGML_QMV_WAVES_SMALLK", 16);                      // ... cap for K <= 2048
    int qmv_kon_waves = env_int("ZGML_QMV_KON_WAVES", 0);                             // waves of the K-on-lanes launches with K > 2048 (0: by K)
    int qmv_kon_waves_smallk = env_int("ZGML_QMV_KON_WAVES_SMALLK", 16);              // ... cap for K <= 2048
    const char* qmv_kon_tune = env_text("ZGML_QMV_KON_TUNE");                         // "<blocks>x<K>:<waves>[:<depth>],...": per launch shape
    bool hip_prenorm_nol = env_flag("ZGML_HIP_PRENORM_NOL", true);                    // the prepared rmsnorm also for x-direct n-on-lanes launches
    bool hip_pair_nol = env_flag("ZGML_HIP_PAIR_NOL", true);                          // the pair launch also for x-direct n-on-lanes launches
    int hip_prenorm_early = env_int("ZGML_HIP_PRENORM_EARLY", 1);                     // 0: the prepared norm's partial sums are folded in the kernel's tail
    int hip_handoff_sleep = env_int("ZGML_HIP_HANDOFF_SLEEP", 2);                     // s_sleep argument between polls of a hand-off counter
    int hip_debug_skip_grid = env_int(trace("ZGML_HIP_DEBUG_SKIP_GRID"), 0);          // leave out every mat-vec launch of this many column groups (timing only)
    bool hip_debug_drop_publish = env_flag(trace("ZGML_HIP_DEBUG_DROP_PUBLISH"), false); // one column group of a fused launch never signals (time-out test)
    // ── K-split layers (ksplit.hip) ──
    int ks_proj_gp = env_int("ZGML_KS_PROJ_GP", 0);                                   // 1 | 2 | 4: column groups per workgroup of the projection (else 2)
    int ks_proj_waves = env_int("ZGML_KS_PROJ_WAVES", 0);                             // waves of the projection launch (0: by K)
    int ks_mlp_waves = env_int("ZGML_KS_MLP_WAVES", 0);                               // waves of the MLP launch (0: by K)
    int ks_debug_a = env_int("ZGML_KS_DEBUG_A", 0);                                   // 1: the attention's workgroups exit at once, 2: they skip the wait (timing only)
    // ── quantized tile kernels, M > 1 (qmatmul_tiles.hip) ──
    bool qmm_xdl2 = env_flag("ZGML_QMM_XDL2", true);                                  // the split-A forms (pre-laid-out A, B-scaled tiles) for Q4_0 with f16 scales
    int qmm_xdl2_g = env_int("ZGML_QMM_XDL2_G", 0);                                   // column groups per workgroup of qmatmul_xdl2_kernel (0: by N)
    bool qmm_xdl4 = env_flag("ZGML_QMM_XDL4", true);                                  // M > 32: the 4 / 8-m-tile K-split kernel
    bool qmm_xdl4_m32 = env_flag("ZGML_QMM_XDL4_M32", true);                          // ... also for narrow M = 17-32 outputs
    int qmm_xdl4_sk = env_int("ZGML_QMM_XDL4_SK", 0);                                 // its K slices (0: to fill the CUs, at most 4)
    bool qmm_xdl5 = env_flag("ZGML_QMM_XDL5", true);                                  // M <= 32: the shared-A kernel for wide outputs
    int qmm_xdl5_wgs_per_cu = env_int("ZGML_QMM_XDL5_WGS_PER_CU", 1);                 // its workgroups per CU (at least 1)
    int qmm_xdl5_min_cols = env_int("ZGML_QMM_XDL5_MIN_COLS", 40);                    // fewest 256-column workgroup-columns it is taken for
    int qmm_xdl5_min_run = env_int("ZGML_QMM_XDL5_MIN_RUN", 2);                       // shortest run of (column, K step) pairs of its work split (at least 1)
    bool qmm_xdl5_trace = env_flag(trace("ZGML_QMM_XDL5_TRACE"), false);              // print the per-phase stamps of its last launch at exit
    int qmm_waves = env_int("ZGML_QMM_WAVES", 8);                                     // most waves per workgroup of the tile kernels
    int qmm_tile_min_m = env_int("ZGML_QMM_TILE_MIN_M", 2);                           // rows from which a quantized matmul takes the tile kernels
    // ── dense f16 (dense_f16.hip) ──
    bool f16_tile2 = env_flag("ZGML_F16_TILE2", true);                                // M > 1: the pre-laid-out-A tile kernel
    bool f16_tile2_wide = env_flag("ZGML_F16_TILE2_WIDE", true);                      // ... 4 / 8 m-tiles per workgroup for M > 32 / 64
    int f16_tile2_waves = env_int("ZGML_F16_TILE2_WAVES", 8);                         // ... most waves per workgroup
    int f16_tile2_cg = env_int("ZGML_F16_TILE2_CG", 0);                               // ... 1 | 2 | 4: column groups per workgroup (0: by the grid)
    int f16_groups = env_int("ZGML_F16_GROUPS", 0);                                   // column groups per workgroup of the plain dense kernel (0: by N)
};

inline const Switches& sw() {
    static const Switches table;
    return table;
}

// ── per-context switches, NOT latched: zgml_hip_create reads them at every call; a variable overrides the option only when set ──
inline bool ctx_flag(const char* name, bool current) { return env_flag(name, current); }
template <typename Ctx>
void read_ctx_switches(Ctx& ctx) {
    ctx.opt_graph = ctx_flag("ZGML_HIP_GRAPH", ctx.opt_graph);       // replay hipGraphs (0: launch the plan eagerly)
    ctx.opt_fusion = ctx_flag("ZGML_HIP_FUSION", ctx.opt_fusion);    // the planner's fusion passes (0: one launch per op)
    ctx.opt_ksplit = ctx_flag("ZGML_HIP_KSPLIT", ctx.opt_ksplit);    // short-K layers as K-split launches (measured slower)
    ctx.opt_w8a8 = ctx_flag("ZGML_HIP_W8A8", ctx.opt_w8a8);          // M = 1 qmatmuls through the reference's W8A8 arithmetic
    ctx.host_prof = ctx_flag("ZGML_HIP_HOST_PROF", ctx.host_prof);   // host time per phase of the vtable path, printed at destroy
}

} // namespace zgml
