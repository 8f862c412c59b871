"""GGUF Q4_K, Q5_K, Q6_K, Q3_K, Q2_K and IQ4_XS (sb_kernels.hip) next to Q4_0 on the same box in the same run: the M = 1 mat-vec against the K-on-lanes
kernel and the M = 32 matmul against the tile kernel, at 4096^2, 4096 x 11008 and 4096 x 32000. Q4_0 and Q4_K stream 4.5 bit/weight,
so their bytes per launch are equal and the times compare directly; Q5_K streams 176/144, Q6_K 210/144, Q3_K 110/144, Q2_K 84/144 and IQ4_XS 136/144 of that, so the GB/s are printed too. A ring of distinct matrices larger than the 256 MiB Infinity Cache
stands for a model; device-event time per launch over replays of a captured graph (zgml_hip_qmatmul_bench); the formats
alternate within each repeat and every repeat is printed, so the spread shows next to the difference.
--rows: the super-block formats at M = 2..8 with ZGML_HIP_OPT_SMALL_M_MATVEC at 8 (the multi-row mat-vecs) and at 0 (the matrix-core
kernel), alternating within each repeat: what the formats' kRowsRoutedM are set by."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, capi  # noqa: E402

FMT = {"q4_0": 1, "q4_k": 2, "q5_k": 4, "q6_k": 3, "q3_k": 5, "q2_k": 6, "iq4_xs": 7}  # the `q4` argument of zgml_hip_qmatmul_bench


def run(be, fmt, M, K, N, ring, iters):
    nbytes = C.c_uint64()
    us = be._lib.zgml_hip_qmatmul_bench(be.ctx, M, K, N, FMT[fmt], ring, 20, iters, C.byref(nbytes))
    if us <= 0:
        raise RuntimeError(be.last_error() or "bench refused the shape")
    return us, nbytes.value


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="4096x4096,4096x11008,4096x32000")
    ap.add_argument("--rows", action="store_true")
    a = ap.parse_args()
    be = Backend(0)
    for shp in a.shapes.split(","):
        K, N = map(int, shp.split("x"))
        ring = max(2, min(64, int(40e9 // (K * N))))
        for M in range(2, 9) if a.rows else ():
            for f in (f for f in FMT if f != "q4_0"):
                us = {"rows": [], "matmul": []}
                for _ in range(a.repeats):
                    for route, value in (("rows", 8), ("matmul", 0)):
                        be.set_option(capi.OPT_SMALL_M_MATVEC, value)
                        try:
                            us[route].append(round(run(be, f, M, K, N, ring, max(64, a.iters // 8))[0], 3))
                        finally:
                            be.set_option(capi.OPT_SMALL_M_MATVEC, 0)
                print(json.dumps({"K": K, "N": N, "M": M, "format": f, "ring": ring, "us": us,
                                  "rows_over_matmul": round(min(us["rows"]) / min(us["matmul"]), 3)}), flush=True)
        for M in () if a.rows else (1, 32):
            us, nbytes = {f: [] for f in FMT}, {}
            for _ in range(a.repeats):
                for f in FMT:
                    t, nbytes[f] = run(be, f, M, K, N, ring, a.iters if M == 1 else max(64, a.iters // 8))
                    us[f].append(round(t, 3))
            best = {f: min(v) for f, v in us.items()}
            print(json.dumps({"K": K, "N": N, "M": M, "ring": ring, "bytes": nbytes, "us": us,
                              "GBps": {f: round(nbytes[f] / best[f] / 1e3, 1) for f in FMT},
                              "q4_k_over_q4_0": round(best["q4_k"] / best["q4_0"], 3),
                              "q6_k_over_q4_k": round(best["q6_k"] / best["q4_k"], 3),
                              "q5_k_over_q4_k": round(best["q5_k"] / best["q4_k"], 3),
                              "q5_k_over_q6_k": round(best["q5_k"] / best["q6_k"], 3),
                              "q3_k_over_q5_k": round(best["q3_k"] / best["q5_k"], 3),
                              "q2_k_over_q5_k": round(best["q2_k"] / best["q5_k"], 3),
                              "iq4_xs_over_q4_k": round(best["iq4_xs"] / best["q4_k"], 3),
                              "iq4_xs_over_q5_k": round(best["iq4_xs"] / best["q5_k"], 3)}), flush=True)
    be.close()
