"""Times the tied LM head alone: a one-op M = 1 dense matmul program over a K-contiguous f32 B (default 576 x 49152, SmolLM-135M's
113 MB head) replayed through zgml_hip_enqueue_program, with HIP events around the replays on the context's stream:
    python tools/head_time.py [K N [replays [rounds]]]
prints microseconds per replay (launch gap included: the same for every build) and the stream rate of B, median and range over
the rounds. The library comes from ZGML_HIP_LIB, so builds are compared by running this once per build, alternating."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from zgml_amd import Backend, DeviceOp, DeviceProgram, MatMulGeometry, ProgramIO, capi  # noqa: E402


def main():
    K, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (576, 49152)
    replays = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    rng = np.random.default_rng(0)
    x = rng.standard_normal(K).astype(np.float32)
    w = (rng.standard_normal(N * K) * 0.05).astype(np.float32)
    g = MatMulGeometry(M=1, N=N, K=K, a_row_stride=K, a_col_stride=1, b_row_stride=1, b_col_stride=K,
                       a_offset=0, b_offset=0, dst_offset=0, dst_row_stride=N)
    prog = DeviceProgram(ops=[DeviceOp.matmul(2, 0, 1, g)], buffer_sizes=[K, N * K, N], initial_uploads=[ProgramIO(0, x), ProgramIO(1, w)])
    be = Backend(0)
    lib = capi.load_hip()
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(lib.zgml_hip_stream(be.ctx))
    h = be.compileProgram(prog)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for _ in range(20):
        lib.zgml_hip_enqueue_program(be.ctx, h)
    be.synchronize()
    us = []
    for _ in range(rounds):
        hip.hipEventRecord(e0, stream)
        for _ in range(replays):
            lib.zgml_hip_enqueue_program(be.ctx, h)
        hip.hipEventRecord(e1, stream)
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        us.append(1e3 * ms.value / replays)
    out = np.zeros(N, np.float32)
    be.executeProgram(h, [], [ProgramIO(2, out)])
    us.sort()
    med = us[len(us) // 2]
    print(f"head {K} x {N} lib={os.environ.get('ZGML_HIP_LIB', 'default')}: {med:.2f} us per replay (range {us[0]:.2f}-{us[-1]:.2f}), "
          f"{4e-6 * K * N / med:.2f} TB/s, checksum {float(np.abs(out).sum()):.6e}", flush=True)
    be.freeProgram(h)
    be.close()


if __name__ == "__main__":
    main()
