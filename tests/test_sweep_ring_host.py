"""The ring of the granule hand-off's wait (zgml_amd/csrc/sweep_ring.h) without a GPU: tests/cpp/sweep_ring_probe.cpp drives it with
a scripted memory for 1 to 4 sweeps in flight. The probe is a stand-alone program built with AddressSanitizer + UBSan and run
directly (as tests/cpp/handoff_gen_probe.cpp is built and run)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PROBE_SRC = ROOT / "tests" / "cpp" / "sweep_ring_probe.cpp"
HEADERS = [ROOT / "zgml_amd" / "csrc" / "sweep_ring.h", ROOT / "zgml_amd" / "csrc" / "handoff_gen.h"]
BUILD = ROOT / "tests" / "cpp" / "_build"


def test_sweep_ring_on_a_scripted_memory():
    """Accepted only from a sweep whose tags all matched, with that sweep's values (the first such sweep issued); a mixed sweep is
    never accepted; the loop ends at the limit and says so; one sweep in flight visits memory as the sequential loop did."""
    exe = BUILD / "sweep_ring_probe"
    BUILD.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or any(p.stat().st_mtime > exe.stat().st_mtime for p in [PROBE_SRC, *HEADERS]):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-o", str(exe), str(PROBE_SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok=1 failures=0", r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
