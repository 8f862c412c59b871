"""The environment switches of libzgml_hip are declared once, in zgml_amd/csrc/switches.h: nothing else in csrc reads the
environment, every name is documented in INTEGRATION.md, the Python side names no switch that nothing reads, and the parse
helpers keep the semantics the read sites had (atoi / base-0 forms, "is set", trace-only rows, the latch on the first sw() call,
the unlatched per-context helper). No GPU: the header is plain C++ and tests/cpp/switches_probe.cpp is built with g++ (as a
program rather than a library: every case needs a fresh process anyway, so that the latch is fresh)."""
import ast
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zgml_amd" / "csrc"
HEADER = CSRC / "switches.h"
PROBE_SRC = ROOT / "tests" / "cpp" / "switches_probe.cpp"
BUILD = ROOT / "tests" / "cpp" / "_build"

# names that other components read: the Python side, the build, the host library, the oracle, test workers
OTHER_COMPONENTS = {
    "ZGML_HIP_LIB", "ZGML_HOST_LIB", "ZGML_ORACLE_LIB", "ZGML_ORACLE_VNNI", "ZGML_SHARD_GATHER", "ZGML_SHARD_FORCE_GATHER",
    "ZGML_BENCH_ONE_GPU", "ZGML_BENCH_FORCE_SHARDED", "ZGML_HOST_SHARD_POINTS_WORLD1", "ZGML_TRACE", "ZGML_KERNARG_PRELOAD",
    "ZGML_PIN_OUTPUTS", "ZGML_TEST_HANDOFF_MODEL",
}


def table_names():
    """every quoted "ZGML_..." in the header, in order (a name that is declared twice appears twice)"""
    return re.findall(r'"(ZGML_[A-Z0-9_]+)"', HEADER.read_text())


def test_one_declaration_documented():
    names = table_names()
    assert len(names) == 83, len(names)
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, f"declared more than once: {dup}"
    for src in sorted(CSRC.iterdir()):
        if src == HEADER or not src.is_file():
            continue
        text = src.read_text()
        for word in ("getenv", "env_int(", "env_flag("):
            assert word not in text, f"{src.name} reads the environment itself ({word})"
        quoted = re.findall(r'"(ZGML_[A-Z0-9_]+)"', text)
        assert not quoted, f"{src.name} names {quoted}: a switch is declared in switches.h only"
    doc = (ROOT / "INTEGRATION.md").read_text()
    missing = [n for n in names if not re.search(rf"\b{n}\b", doc)]
    assert not missing, f"not in INTEGRATION.md: {missing}"
    # a trace-only row is marked as such in the table of section 9
    trace_only = re.findall(r'trace\("(ZGML_[A-Z0-9_]+)"\)', HEADER.read_text())
    assert len(trace_only) == 5, trace_only
    unmarked = [n for n in trace_only if not re.search(rf"`{n}[^`]*` \(trace\)", doc)]
    assert not unmarked, f"trace-only but not marked (trace) in INTEGRATION.md: {unmarked}"


def python_side_names():
    """ZGML_* names the Python side hands to a process environment: string literals that are exactly a name (or NAME=value) —
    os.environ[...] / env dictionaries / monkeypatch.setenv / tuples of names — and keyword names (dict(os.environ, ZGML_X="1"))"""
    files = sorted((ROOT / "tests").glob("*.py")) + sorted((ROOT / "tools").glob("*.py")) + sorted((ROOT / "zgml_amd").glob("*.py"))
    files += [ROOT / "bench.py", ROOT / "__graft_entry__.py"]
    pat = re.compile(r"(ZGML_[A-Z0-9_]+)(=.*)?")
    found = {}
    for f in files:
        if f.name == "test_switches.py":
            continue
        for node in ast.walk(ast.parse(f.read_text())):
            name = None
            if isinstance(node, ast.Constant) and isinstance(node.value, str):
                m = pat.fullmatch(node.value)
                name = m.group(1) if m else None
            elif isinstance(node, ast.keyword) and node.arg and node.arg.startswith("ZGML_"):
                name = node.arg
            if name:
                found.setdefault(name, set()).add(f.name)
    return found


def test_no_stray_names():
    found = python_side_names()
    assert "ZGML_QMM_XDL5_MIN_COLS" in found and "ZGML_SHARD_PEER_WAIT_MS" in found and "ZGML_HIP_QMV_KON" in found  # (the scan sees all three forms)
    known = set(table_names()) | OTHER_COMPONENTS
    stray = {n: sorted(fs) for n, fs in found.items() if n not in known}
    assert not stray, f"names that no component reads (misspelt?): {stray}"


def probe(trace):
    exe = BUILD / ("switches_probe_trace" if trace else "switches_probe")
    BUILD.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in (PROBE_SRC, HEADER)):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *(["-DZGML_TRACE"] if trace else []), "-o", str(exe), str(PROBE_SRC)],
                       check=True)
    return exe


def run(env=None, after=None, trace=False):
    """-> {tag: {field: text}} of one probe process whose environment holds only `env` of the ZGML_* names"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("ZGML_")}
    r = subprocess.run([str(probe(trace)), *(after or ())], env={**base, **(env or {})}, capture_output=True, text=True, check=True)
    out = {}
    for line in r.stdout.splitlines():
        tag, *fields = line.split()
        out[tag] = dict(f.split("=", 1) for f in fields)
    return out


def test_defaults_when_unset():
    for trace in (False, True):
        o = run(trace=trace)
        assert o["first"] == {"qmv_xdirect": "1", "qmm_waves": "8", "hip_nt_min_bytes": str(192 << 20), "copy_variant": str(8 | 1 << 8 | 32 << 16),
                              "hip_elt_vec4_min": str(1 << 20), "debug_plan_set": "0", "debug_plan": "0", "qmm_xdl5_trace": "0",
                              "hip_debug_skip_grid": "0", "hip_skip_kinds": "0", "graph_dump": "(null)"}
        assert o["ctx_first"] == {"graph": "1", "fusion": "1", "ksplit": "0", "w8a8": "0", "host_prof": "0"}


@pytest.mark.parametrize("text,flag,num", [("0", "0", "0"), ("1", "1", "1"), ("7", "1", "7")])
def test_flag_and_int(text, flag, num):
    o = run({"ZGML_QMV_XDIRECT": text, "ZGML_QMM_WAVES": text})["first"]
    assert o["qmv_xdirect"] == flag and o["qmm_waves"] == num


def test_base0_and_atoi_rows():
    o = run({"ZGML_HIP_NT_MIN_BYTES": "0x10", "ZGML_COPY_VARIANT": "0x10", "ZGML_QMM_WAVES": "0x10", "ZGML_QMV_XDIRECT": "0x10",
             "ZGML_HIP_ELT_VEC4_MIN": "64", "ZGML_HIP_GRAPH_DUMP": "/tmp/d"})["first"]
    assert o["hip_nt_min_bytes"] == "16" and o["copy_variant"] == "16"  # strtoull / strtol, base 0
    assert o["qmm_waves"] == "0" and o["qmv_xdirect"] == "0"              # atoi stops at the x
    assert o["hip_elt_vec4_min"] == "64" and o["graph_dump"] == "/tmp/d"
    assert run({"ZGML_HIP_ELT_VEC4_MIN": "0x10"})["first"]["hip_elt_vec4_min"] == "0"  # atol


def test_debug_plan_is_set_even_at_zero():
    o = run({"ZGML_HIP_DEBUG_PLAN": "0"})["first"]
    assert o["debug_plan_set"] == "1" and o["debug_plan"] == "0"
    o = run({"ZGML_HIP_DEBUG_PLAN": "2"})["first"]
    assert o["debug_plan_set"] == "1" and o["debug_plan"] == "2"


def test_trace_only_rows():
    env = {"ZGML_QMM_XDL5_TRACE": "1", "ZGML_HIP_DEBUG_SKIP_GRID": "36", "ZGML_HIP_SKIP_KINDS": "0x10"}
    o = run(env, trace=False)["first"]
    assert (o["qmm_xdl5_trace"], o["hip_debug_skip_grid"], o["hip_skip_kinds"]) == ("0", "0", "0")  # the product build does not look
    o = run(env, trace=True)["first"]
    assert (o["qmm_xdl5_trace"], o["hip_debug_skip_grid"], o["hip_skip_kinds"]) == ("1", "36", "16")


def test_latched_on_first_use():
    o = run({"ZGML_QMM_WAVES": "3"}, after=("ZGML_QMM_WAVES", "5"))
    assert o["first"]["qmm_waves"] == "3" and o["second"]["qmm_waves"] == "3"
    o = run(after=("ZGML_QMV_XDIRECT", "0"))  # unset at the first call: the default stays
    assert o["first"]["qmv_xdirect"] == "1" and o["second"]["qmv_xdirect"] == "1"


def test_context_switches_are_read_at_every_call():
    o = run(after=("ZGML_HIP_GRAPH", "0"))
    assert o["ctx_first"]["graph"] == "1" and o["ctx_second"]["graph"] == "0"
    o = run({"ZGML_HIP_KSPLIT": "1", "ZGML_HIP_FUSION": "0"}, after=("ZGML_HIP_KSPLIT", "0"))
    assert o["ctx_first"] == {"graph": "1", "fusion": "0", "ksplit": "1", "w8a8": "0", "host_prof": "0"}
    assert o["ctx_second"] == {"graph": "1", "fusion": "0", "ksplit": "0", "w8a8": "0", "host_prof": "0"}  # unset ones keep what they were given
