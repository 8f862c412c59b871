"""The native CPU code (oracle C restatement with its pthread pools, C++ host mirror) under AddressSanitizer + UBSan and
under ThreadSanitizer: tools/run_sanitizers.sh builds the instrumented libraries (oracle/Makefile SAN=..., build_host(san=...))
and re-runs the CPU tests that drive them in a child interpreter with the sanitizer runtime preloaded. Never the GPU side
(device sanitizers are not available on the pool). Reference precedent: src/thread_pool.zig:180-199."""
import os
import platform
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _tsan_cannot_start():
    """Why GCC's ThreadSanitizer runtime cannot start an interpreter on this machine (None: it can). It needs every mapping of
    the process inside its application ranges; where the address-space layout puts one elsewhere and address randomisation
    cannot be switched off for a child, it dies at start-up ("unexpected memory mapping") before any test code runs. Three
    tries, as tools/run_sanitizers.sh starts its interpreter (setarch -R where permitted)."""
    rt = subprocess.run(["gcc", "-print-file-name=libtsan.so"], capture_output=True, text=True).stdout.strip()
    norand = ["setarch", platform.machine(), "-R"]
    if subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    pre = os.environ.get("LD_PRELOAD")
    env = dict(os.environ, LD_PRELOAD=rt + (" " + pre if pre else ""), TSAN_OPTIONS="halt_on_error=1")
    for _ in range(3):
        r = subprocess.run(norand + ["python3", "-c", "pass"], env=env, capture_output=True, text=True, timeout=120)
        if "unexpected memory mapping" in r.stderr:
            return r.stderr.strip().splitlines()[-1]
    return None


@pytest.mark.timeout(900)
@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_cpu_native_code_under_sanitizer(san):
    why = _tsan_cannot_start() if san == "tsan" else None
    if why:
        pytest.skip("ThreadSanitizer cannot start a process on this machine: " + why)
    r = subprocess.run([str(ROOT / "tools" / "run_sanitizers.sh"), san], capture_output=True, text=True, timeout=880)
    assert r.returncode == 0 and "SANITIZERS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
