"""The block map of the fused q / k / v + decode attention launch (zgml_amd/csrc/qkv_colocate.h) without a GPU: which block id plays
which role, so that a kv group's projection column groups and split 0 of its heads carry one label `block id % 8` (blocks of one
label share an XCD where the dispatcher deals them as observed; nothing but speed depends on it).

tests/cpp/qkv_colocate_probe.cpp evaluates the role of every block id of every case and reports the properties; it is built as a
stand-alone program with AddressSanitizer + UBSan."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PROBE_SRC = ROOT / "tests" / "cpp" / "qkv_colocate_probe.cpp"
HEADER = ROOT / "zgml_amd" / "csrc" / "qkv_colocate.h"
BUILD = ROOT / "tests" / "cpp" / "_build"

# (n_heads, n_kv, d_head, n_sp) -> does every label hold the kv groups dealt to it? (worked out by hand: a group needs
# (n_heads / n_kv + 2) d_head / 16 + n_heads / n_kv ids, label l of a grid of G ids has (G - l + 7) // 8)
CASES = {
    (9, 3, 64, 16): True,     # SmolLM-135M: 23 per group, 204 ids, 25-26 per label
    (9, 3, 64, 1): False,     # ... with one split: 69 ids, 8-9 per label
    (32, 32, 128, 2): True,   # 25 per group, four groups per label: 100 of 104
    (32, 8, 128, 4): True,    # 52 per group, 512 ids, 64 per label
    (4, 1, 64, 16): False,    # 28 for the one group, 88 ids, 11 per label
    (12, 12, 64, 8): True,    # 13 per group, two groups on labels 0-3: 26 of 30
    (64, 8, 128, 1): True,    # 88 per group, 704 ids: exactly 88 per label, nothing left over
    (6, 6, 128, 16): True,    # tests/test_hip_qkv_colocate.py's d_head 128 model: 25 per group, 240 ids
    (6, 6, 128, 1): False,    # ... with one split: 150 ids, 18-19 per label
    (9, 3, 64, 8): False,     # SmolLM's layer with 8 splits: 132 ids, 16-17 per label
}


@pytest.fixture(scope="module")
def probe():
    exe = BUILD / "qkv_colocate_probe"
    BUILD.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(p.stat().st_mtime > exe.stat().st_mtime for p in (PROBE_SRC, HEADER)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", str(exe), str(PROBE_SRC)], check=True)
    return exe


def _rows(exe, cases=None):
    args = [str(v) for c in (cases or []) for v in c]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split())
        if "case" in f:
            rows[tuple(int(v) for v in f["case"].split(","))] = {k: int(v) for k, v in f.items() if k != "case"}
    return r, rows


def test_the_probes_own_table(probe):
    """the probe's built-in table is the first seven cases, and it passes its own checks (exit status) under the sanitizers"""
    r, rows = _rows(probe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert list(rows) == list(CASES)[:7]
    assert r.stdout.splitlines()[-1] == "ok=1"


@pytest.mark.parametrize("case", list(CASES))
def test_map_properties(probe, case):
    r, rows = _rows(probe, [case])
    assert r.returncode == 0, r.stdout + r.stderr
    f = rows[case]
    n_heads, n_kv, d_head, n_sp = case
    assert f["grid"] == (n_heads + 2 * n_kv) * d_head // 16 + n_heads * n_sp  # the grid is not padded
    assert f["bijection"] == 1 and f["packed"] == 1
    assert f["fits"] == int(CASES[case])
    if CASES[case]:  # the groups fit: co-located, the projection first on every label
        assert f["on"] == 1 and f["identity"] == 0
        assert f["colocated"] == 1 and f["ordered"] == 1
    else:  # they do not: the launch is what it was
        assert f["on"] == 0 and f["identity"] == 1
