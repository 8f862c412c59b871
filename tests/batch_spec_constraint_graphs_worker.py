"""Worker of tests/test_hip_batch_spec_constraint.py: which graphs the batched speculative calls capture on one program, in a process
of its own because the graph dump (ZGML_HIP_GRAPH_DUMP, set by the test) is read once per process. It names every phase on stderr,
where the library names the graphs it captures; the test reads the order."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from zgml_amd import Backend, capi, llama  # noqa: E402


def main():
    be = Backend(0)
    cfg = llama.preset("tiny", 64)
    V, B, Ts, n = cfg.vocab_size, 2, 4, 9
    bm = llama.BatchModel(cfg, B, llama.Q4_0, tokens_per_seq=Ts)
    s = llama.BatchSession(bm, llama.hip_backend_fns(be), B)
    s.resident_setup(be)
    con = be.constraint_create(np.zeros(V, np.uint16), np.zeros((1, 1), np.uint16))  # one state, every token allowed
    sps = [capi.SamplingC.of(0.8, 40, 0.95, seed=b + 1, stream=b) for b in range(B)]
    args = ([3, 90], [0, 0], [n, n])

    def phase(name):
        be.synchronize()
        print("PHASE " + name, file=sys.stderr, flush=True)

    def attach(on):
        s.set_constraint(con if on else None, 0, seq=1)

    def call(name):
        attach(name.startswith("attached"))
        if name == "greedy":
            s.resident_decode_batch_speculative(*args)
        elif name == "sampled":
            s.resident_decode_batch_speculative_sampled(*args, sps)
        else:  # detached, attached, attached_logprobs
            s.resident_decode_batch_speculative_constrained(*args, sps, logprobs=True if name.endswith("logprobs") else None)
        assert not be.last_error(), be.last_error()

    names = ["sampled", "detached", "attached", "attached_logprobs", "greedy"]
    for name in names:
        phase(name)
        call(name)
    phase("settle")  # (the first `logprobs` call allocated the values' table, which drops the graphs captured before it: they come back here)
    for name in names:
        call(name)
    phase("again")
    for name in names[::-1] + names:
        call(name)
    phase("end")
    attach(False)
    be.constraint_free(con)
    s.close(), bm.close(), be.close()
    print("BATCH_SPEC_CONSTRAINT_GRAPHS_OK")


if __name__ == "__main__":
    main()
