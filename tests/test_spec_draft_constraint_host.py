"""CPU tests of speculative decode with a draft model under a constraint (include/zgml_hip.h:
zgml_hip_resident_decode_speculative_model_constrained). The rule is zgml_amd/csrc/spec.h (DRAFTS FROM A MODEL UNDER A CONSTRAINT:
spec_masked_first_max, spec_draft_advance_constrained, spec_candidates_model_constrained) — the functions the kernels call —,
reached through tests/cpp/spec_draft_constraint_probe.cpp. Every comparison is exact equality of integers.

1. The header against the model tests/spec_draft_constraint_model.py: seeded, template and chain automata, random draft rows with
   ties and -inf runs, n_classes = 1 and 8192 (empty classes), vocabularies that are no multiple of 256, T in {2, 4, 5}: equal c,
   row_state and `drafted`.
2. Properties: a forcing state drafts forced[s] whatever the row holds; behind a live state that allows a token the next row is
   never dead; behind a dead or empty state every later row is dead and c repeats.
3. The whole loop on the oracle with the tiny model: draft A under a seeded automaton and top_k = 1 is accepted in full; the same
   loop without the mask is accepted strictly less and drafts a forbidden token in at least one step; the streams are equal.
4. The probe's stand-alone program under AddressSanitizer + UBSan.
5. The entry point is exported and declared in the ctypes mirror."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from zgml_amd import capi, llama
from tests import spec_constraint_model as SCM
from tests import spec_draft_constraint_model as SDM
from tests.test_constraint_host import Dfa, FORBIDDEN, c_constraint_sample, random_dfa
from tests.test_hip_constraint import seeded_dfa
from tests.test_spec_constraint_host import chain_dfa, template_dfa
from tests.test_spec_draft_model_host import FIRST, N, target_cfg

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libspec_draft_constraint_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "spec_draft_constraint_probe.cpp", ROOT / "zgml_amd" / "csrc" / "spec.h", ROOT / "zgml_amd" / "csrc" / "sample.h",
        ROOT / "zgml_amd" / "csrc" / "sample_params.h", ROOT / "include" / "zgml_hip.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "include")]
f32, u16, u32 = np.float32, np.uint16, np.uint32
S = capi.SamplingC.of
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", *FLAGS, "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, w = C.c_void_p, C.c_uint32
    lib.sdc_dead.argtypes, lib.sdc_dead.restype = [], w
    lib.sdc_no_forced.argtypes, lib.sdc_no_forced.restype = [], w
    lib.sdc_masked_first_max.argtypes, lib.sdc_masked_first_max.restype = [vp, w, w, vp, vp, w], C.c_int64
    lib.sdc_candidates.argtypes, lib.sdc_candidates.restype = [w, w, w, w, vp, vp, w, vp, vp, vp, vp], w
    _lib = lib
    return lib


def c_masked_first_max(row, dfa, state):
    row = np.ascontiguousarray(row, f32)
    return int(probe().sdc_masked_first_max(row.ctypes.data, row.size, state, dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes))


def c_candidates(tok, T, state, dfa, rows):
    """the header's step over the draft rows rows[T - 1][vocab] -> (c, row_state, drafted, the rows it asked for)"""
    rows = np.ascontiguousarray(rows, f32).reshape(T - 1, dfa.class_of.size)
    c, row_state, asked = np.zeros(T, u32), np.zeros(T, u32), np.zeros(T, u32)
    drafted = probe().sdc_candidates(tok, T, dfa.class_of.size, state, dfa.class_of.ctypes.data, dfa.next.ctypes.data, dfa.n_classes, rows.ctypes.data,
                                     c.ctypes.data, row_state.ctypes.data, asked.ctypes.data)
    return c.tolist(), row_state.tolist(), int(drafted), asked[:T - 1].tolist()


def model_candidates(tok, T, state, dfa, rows):
    c, row_state, drafted, _ = SDM.draft_candidates(tok, T, state, dfa.class_of, dfa.next, lambda j, c: rows[j] if j < T - 1 else None)  # (the T-th row is dropped)
    return c, row_state, drafted


def draft_rows(rng, T, vocab):
    """random rows of few distinct values (ties), some with runs of -inf, one now and then -inf everywhere"""
    rows = (rng.integers(0, 24, (T, vocab)) / 4.0).astype(f32)
    for r in rows:
        kind = rng.integers(0, 4)
        if kind == 0:
            at = int(rng.integers(0, vocab))
            r[at:at + int(rng.integers(1, vocab + 1))] = -np.inf
        elif kind == 1:
            r[rng.random(vocab) < 0.7] = -np.inf
    if rng.random() < 0.1:
        rows[int(rng.integers(0, T))] = -np.inf
    return rows


def test_the_sentinels_are_the_models():
    assert (probe().sdc_dead(), probe().sdc_no_forced()) == (SCM.DEAD, SCM.NO_FORCED) and SCM.DEAD == FORBIDDEN


# ── 1. the header against the model ────────────────────────────────────────────────────────────────────────────────────

def automata():
    """(name, Dfa) over vocabularies that are no multiple of 256; n_classes 1 and 8192 among them"""
    rng = np.random.default_rng(271)
    out = [("seeded-%d" % seed, seeded_dfa(seed, 515)) for seed in (3, 11)]
    out += [("seeded-one-state", seeded_dfa(5, 300, n_states=1, n_classes=3))]
    out += [("template", template_dfa(515, [0, 1, 0, 3, 0, 6], seed=21)[0]), ("template-runs-only", template_dfa(130, [2, 2], free_classes=1, seed=4)[0])]
    out += [("chain-free", chain_dfa(67, 5)), ("chain-forced", chain_dfa(67, 9, token_of=lambda s: (7 * s + 1) % 67))]
    out += [("one-class", Dfa(np.zeros(259, u16), np.array([[1], [FORBIDDEN], [0]], u16)))]  # every token, no token, every token
    wide = random_dfa(rng, 1030, n_states=4, n_classes=8192, forbid=0.5)  # 1030 tokens in 8192 classes: most classes are empty
    assert np.unique(wide.class_of).size < 1030 < 8192
    out += [("8192-classes", wide), ("8192-classes-sparse", random_dfa(rng, 777, n_states=3, n_classes=8192, forbid=0.995))]
    out += [("random-%d" % i, random_dfa(rng, int(rng.integers(1, 700)), n_states=int(rng.integers(1, 7)), n_classes=int(rng.integers(1, 50)),
                                         forbid=float(rng.choice([0.3, 0.8, 0.97])))) for i in range(30)]
    return out


@pytest.mark.parametrize("T", [2, 4, 5])
def test_candidates_match_the_model(T):
    rng = np.random.default_rng(100 + T)
    seen = {"dead_start": 0, "no_token": 0, "all_live": 0, "inf_row_drafted": 0, "tie": 0}
    for name, dfa in automata():
        vocab = dfa.class_of.size
        for case in range(12):
            rows = draft_rows(rng, T - 1, vocab)
            state = SCM.DEAD if case == 0 else int(rng.integers(0, dfa.n_states))
            tok = int(rng.integers(0, vocab))
            want = model_candidates(tok, T, state, dfa, rows)
            got = c_candidates(tok, T, state, dfa, rows)
            assert got[:3] == want, (name, case)
            c, row_state, drafted = want
            assert got[3] == [int(s != SCM.DEAD) for s in row_state[:T - 1]]  # a row behind a dead state is not read
            assert drafted == sum(s != SCM.DEAD for s in row_state[1:])
            seen["dead_start"] += state == SCM.DEAD
            seen["no_token"] += any(row_state[j] != SCM.DEAD and row_state[j + 1] == SCM.DEAD for j in range(T - 1))
            seen["all_live"] += SCM.DEAD not in row_state
            for j in range(T - 1):
                if row_state[j + 1] == SCM.DEAD:
                    continue
                seen["inf_row_drafted"] += bool(np.all(np.isneginf(rows[j][dfa.allowed(row_state[j])])))
                seen["tie"] += int(np.sum(rows[j][dfa.allowed(row_state[j])] == rows[j][c[j + 1]])) > 1
    print(T, seen)
    assert all(v >= 10 for v in seen.values()), seen


def test_masked_first_max_by_hand():
    # tokens 0..5; classes 0 = {0, 1}, 1 = {2}, 2 = {} (empty), 3 = {3}, 4 = {4, 5}
    F = FORBIDDEN
    dfa = Dfa([0, 0, 1, 3, 4, 4], np.array([[F, F, F, F, F], [F, 0, F, F, F], [F, F, 0, F, F], [0, F, F, F, 0], [0, 0, 0, 0, 0]], u16))
    inf = np.inf
    for fn in (lambda row, s: c_masked_first_max(row, dfa, s), lambda row, s: SDM.masked_first_max(np.asarray(row, f32), dfa.class_of, dfa.next, s)):
        assert fn([9, 8, 7, 6, 5, 4], 0) == -1                   # no class allowed
        assert fn([9, 8, 7, 6, 5, 4], 2) == -1                   # the empty class alone
        assert fn([9, 8, -inf, 6, 5, 4], 1) == 2                 # forced, over -inf
        assert fn([1, 1, 9, 9, 1, 1], 3) == 0                    # the forbidden maxima contribute nothing; lower index among equals
        assert fn([1, 2, 9, 9, 2, 1], 3) == 1
        assert fn([-inf, -inf, 9, 9, -inf, -inf], 3) == 0        # nothing beats the first allowed token
        assert fn([-inf, -inf, 9, 9, -inf, 0], 3) == 5
        assert fn([3, 3, 3, 3, 3, 3], 4) == 0 and fn([0, 0, 0, 7, 7, 0], 4) == 3


# ── 2. properties ──────────────────────────────────────────────────────────────────────────────────────────────────────

def test_a_forcing_state_drafts_its_forced_token_whatever_the_row_holds():
    rng = np.random.default_rng(5)
    n_forcing = 0
    for name, dfa in automata():
        frc = SCM.forced(dfa.class_of, dfa.next)
        vocab = dfa.class_of.size
        for s in range(dfa.n_states):
            if frc[s] == SCM.NO_FORCED:
                continue
            n_forcing += 1
            for row in (draft_rows(rng, 1, vocab)[0], np.full(vocab, -np.inf, f32), np.zeros(vocab, f32)):
                assert c_masked_first_max(row, dfa, s) == frc[s], (name, s)
                c, row_state, drafted, _ = c_candidates(3 % vocab, 2, s, dfa, row[None, :])
                assert c[1] == frc[s] and row_state[1] == dfa.advance(s, frc[s]) != SCM.DEAD and drafted == 1
    assert n_forcing >= 10 + 4 + 8  # at least the literal states of the two templates and the forced chain's live states
    # a fully forced chain is drafted as it stands, T - 1 tokens per step, over rows that say something else
    chain = chain_dfa(67, 9, token_of=lambda s: (7 * s + 1) % 67)
    rows = np.zeros((4, 67), f32)
    rows[:, 66] = 5.0
    assert c_candidates(0, 5, 2, chain, rows)[:3] == ([0, 15, 22, 29, 36], [2, 3, 4, 5, 6], 4)


def test_live_rows_stay_live_and_dead_rows_stay_dead():
    rng = np.random.default_rng(6)
    seen = {"live_behind_live": 0, "dead_behind_empty": 0, "dead_behind_dead": 0}
    for name, dfa in automata():
        vocab = dfa.class_of.size
        for case in range(20):
            T = int(rng.choice([2, 4, 5]))
            c, row_state, drafted, _ = c_candidates(int(rng.integers(0, vocab)), T, int(rng.integers(0, dfa.n_states)), dfa, draft_rows(rng, T - 1, vocab))
            for j in range(T - 1):
                s = row_state[j]
                if s != SCM.DEAD and dfa.allowed(s).any():  # behind a live state that allows a token the next row is never dead
                    assert row_state[j + 1] != SCM.DEAD and dfa.allowed(s)[c[j + 1]] and row_state[j + 1] == dfa.advance(s, c[j + 1]), (name, case)
                    seen["live_behind_live"] += 1
                else:  # behind a dead or an empty state every later row is dead, and c repeats
                    assert all(x == SCM.DEAD for x in row_state[j + 1:]) and all(x == c[j] for x in c[j + 1:]), (name, case)
                    seen["dead_behind_dead" if s == SCM.DEAD else "dead_behind_empty"] += 1
    assert all(v >= 20 for v in seen.values()), seen


# ── 3. the loop on the oracle ──────────────────────────────────────────────────────────────────────────────────────────

SEED_DFA = 9   # of the seeded automaton: chosen from the oracle's loops alone (the unmasked draft is forbidden in some step), then left fixed
STATE0 = 1
GAP = 1e-3     # the tie bar of tests/test_spec_draft_model_host.py, here between the two best ALLOWED logits of every draft row that drafts


class Pair:
    """the two sessions on the oracle — draft A: the target's own configuration — and what the loop needs of them"""

    def __init__(self, oracle, T, dfa, sp):
        self.T, self.cfg, self.dfa, self.sp = T, target_cfg(), dfa, sp
        self.tm = llama.Model(self.cfg, llama.Q4_0, token_len=T)
        self.ts = llama.Session(self.tm, oracle.backend_fns())
        self.dm = llama.Model(self.cfg, llama.Q4_0)
        self.ds = llama.Session(self.dm, oracle.backend_fns())
        self.ob = oracle.OracleBackend()

    def rows(self, c, pos, row_state, known):
        V = self.cfg.vocab_size
        self.ts.prefill(c, pos, want_logits=False)
        logits = self.ob.buffer(self.ts.handle, self.tm.buf("logits"))[:self.T * V].reshape(self.T, V)
        g = []
        for j in range(self.T):
            tok = -1 if row_state[j] == SCM.DEAD else c_constraint_sample(logits[j], self.sp, pos + j, known + c[1:j + 1], self.dfa, row_state[j])[0]
            g.append(tok if tok >= 0 else SCM.NO_PICK)
        return g

    def draft(self, tok, pos):
        return self.ds.step(tok, pos)[1]

    def loop(self, n, **kw):
        return SDM.spec_loop(self.rows, self.draft, FIRST, 0, n, self.T, self.dfa.class_of, self.dfa.next, STATE0, **kw)

    def close(self):
        for x in (self.ts, self.tm, self.ds, self.dm):
            x.close()


@pytest.mark.parametrize("T", [2, 4, 5])
def test_masked_draft_a_is_accepted_in_full_and_the_unmasked_one_is_not(oracle, T):
    cfg = target_cfg()
    dfa = seeded_dfa(SEED_DFA, cfg.vocab_size)
    sp = S(1.0, 1, 1.0, seed=3)  # top_k = 1: the greedy form of the constrained pick
    gaps, forbidden_drafts = [], []

    def masked_step(pos, c, row_state, g, a, m, rows):
        for j in range(T - 1):
            if row_state[j + 1] != SCM.DEAD:
                best = np.sort(rows[j][dfa.allowed(row_state[j])].astype(np.float64))[-2:]
                gaps.append(float(best[-1] - best[0]) / float(np.abs(rows[j]).max()))

    def unmasked_step(pos, c, row_state, g, a, m, rows):
        forbidden_drafts.append(any(row_state[j] != SCM.DEAD and row_state[j + 1] == SCM.DEAD for j in range(T - 1)))

    p = Pair(oracle, T, dfa, sp)
    toks, produced, stats, state = p.loop(N, on_step=masked_step)
    p.close()
    steps = -(-N // T)
    assert produced == N and -1 not in toks
    assert stats == {"steps": steps, "drafted": steps * (T - 1), "accepted": steps * (T - 1)}, stats
    assert min(gaps) >= GAP, min(gaps)  # no near-tie among the allowed logits decided a draft
    walk = STATE0
    for t in toks:
        walk = dfa.advance(walk, t)
        assert walk != SCM.DEAD
    assert walk == state
    p = Pair(oracle, T, dfa, sp)
    toks_u, produced_u, stats_u, state_u = p.loop(N, mask=False, on_step=unmasked_step)
    p.close()
    print(T, stats, stats_u, sum(forbidden_drafts))
    assert (toks_u, produced_u, state_u) == (toks, produced, state)  # drafts never change tokens
    assert stats_u["accepted"] < stats["accepted"] and stats_u["steps"] > stats["steps"]
    assert any(forbidden_drafts)  # a step whose unmasked draft its row's state forbids


# ── 4. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "spec_draft_constraint_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSPEC_DRAFT_CONSTRAINT_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "spec_draft_constraint_probe ok" in r.stdout, r.stdout + r.stderr


# ── 5. the ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────────

def test_entry_point_is_exported_and_mirrored():
    if not capi.HIP_LIB_PATH.exists():
        import __graft_entry__ as g
        g.build_hip()
    lib = capi.load_hip()
    name = "zgml_hip_resident_decode_speculative_model_constrained"
    assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
    assert getattr(lib, name).argtypes == lib.zgml_hip_resident_decode_speculative_model.argtypes  # the signature of the sibling
    assert name in (ROOT / "include" / "zgml_hip.h").read_text()
    assert hasattr(llama.Session, "resident_decode_speculative_model_constrained")
