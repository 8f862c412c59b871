"""SHA-256 of every weight the host model builder makes for the file-block kinds (3-15): the qweight bytes of a gguf kind, the f32
weight uploads of a dense kind, on preset("tiny") and on the all-256 config of the super-block tests. Two builds of the host
library that print the same lines build the same synthetic models. No GPU."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from zgml_amd import llama  # noqa: E402


def all_256():
    cfg = llama.preset("tiny")
    cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.d_ff, cfg.vocab_size, cfg.n_layers, cfg.tied_lm_head = 256, 4, 4, 512, 512, 2, 0
    return cfg


for name, cfg in (("tiny", llama.preset("tiny")), ("all-256", all_256())):
    for kind in range(3, 16):
        m = llama.Model(cfg, kind)
        p, n = m.program, 7 * cfg.n_layers + (not cfg.tied_lm_head)
        blobs = [(q.data, q.data_len) for q in p.qweights[:p.n_qweights]] or [(u.host_ptr, u.size) for u in p.initial_uploads[:n]]
        assert len(blobs) == n
        for i, (ptr, nbytes) in enumerate(blobs):
            print(name, kind, i, nbytes, hashlib.sha256(C.string_at(ptr, nbytes)).hexdigest())
        m.close()
