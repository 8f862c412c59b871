"""The diagnostics build's counters of the granule hand-off's wait (attention_decode.h, -DZGML_TRACE only): with
ZGML_HIP_ATTN_TRACE=1 every traced workgroup of a fused q / k / v + decode attention launch records, next to its eight stamps,
how many sweeps its wait checked and the round trip of the first one; zgml_hip_free_program prints them. They are what
profiles/r30_sweep_ring.txt was measured with. The switch is read once per process, so the decode runs in a child process on the
diagnostics library (a reduced SmolLM: 2 layers, vocabulary 2048, max_seq 256: 2 launches x 3 kv groups = 6 records)."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TRACE_LIB = ROOT / "zgml_amd" / "lib" / "libzgml_hip_trace.so"

CHILD = f"""
import sys
sys.path.insert(0, {str(ROOT)!r})
from zgml_amd import Backend, llama
be = Backend(0)
cfg = llama.preset("smollm-135m", 256)
cfg.n_layers, cfg.vocab_size = 2, 2048
m = llama.Model(cfg, llama.Q4_0, threads=8)
s = llama.Session(m, llama.hip_backend_fns(be))
toks, _ = s.decode(3, 0, 24)
assert not be.last_error(), be.last_error()
print("TOKENS", toks.tolist())
s.close(), m.close(), be.close()
"""


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("ZGML_HIP_FUSE_QKV_ATTN") == "0", reason="the diagnostic switch turns the fused launch off")
def test_trace_build_prints_sweep_counters():
    assert TRACE_LIB.exists(), "run __graft_entry__.build(): it builds the diagnostics library too"
    env = dict(os.environ, ZGML_HIP_LIB=str(TRACE_LIB), ZGML_HIP_ATTN_TRACE="1")
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "TOKENS" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    recs = re.findall(r"^\s+L\d+ gap\s+-?\d+ \|(?:\s+-?\d+){7} \| sweeps\s+(\d+) first-rtt\s+(\d+)$", r.stderr, re.M)
    print(r.stderr[-1500:])
    assert len(recs) == 6, r.stderr[-4000:]
    for sweeps, rtt in recs:
        # a wait that ends is some sweeps long, far below the give-up limit (400000), and a round trip to memory is neither
        # free nor anywhere near a millisecond (the wall clock ticks in 10 ns)
        assert 1 <= int(sweeps) < 1000, recs
        assert 100 <= int(rtt) < 1000000, recs
