"""CPU tests of zgml_amd/csrc/dev_block.h — the owner of every device block of the resident state and the all-or-nothing ensure
of a group of them — over a counting malloc / free that fails at a chosen call (tests/cpp/dev_block_probe.cpp, g++ -Wall -Werror):

1. ensure: allocates when empty, keeps for a smaller or equal count, moves for a larger one, and is EMPTY after a failed regrow.
2. The group of five blocks of mixed element sizes: fail the j-th allocation, for every j — all five empty, allocations made ==
   frees made; the retry fills all five; members that hold enough are left alone.
3. Move leaves the source empty; destruction frees exactly once.
4. A count whose byte size overflows size_t is refused with no call of the allocator.
5. The probe's stand-alone program under AddressSanitizer + UBSan (leaks and double frees of real memory).
Every comparison is exact."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "_build"
LIB = BUILD / "libdev_block_probe.so"
SRCS = [ROOT / "tests" / "cpp" / "dev_block_probe.cpp", ROOT / "zgml_amd" / "csrc" / "dev_block.h"]
FLAGS = ["-std=c++17", "-Wall", "-Werror"]
K = 5
FAILED, KEPT, MOVED = 0, 1, 2
SIZE_MAX = 2 ** (8 * C.sizeof(C.c_size_t)) - 1
_lib = None


def probe():
    global _lib
    if _lib is not None:
        return _lib
    BUILD.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRCS):
        subprocess.run(["g++", "-O1", *FLAGS, "-shared", "-fPIC", "-o", str(LIB), str(SRCS[0])], check=True)
    lib = C.CDLL(str(LIB))
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    lib.c_mem_reset.argtypes, lib.c_mem_reset.restype = [C.c_int64], None
    lib.c_mem_counts.argtypes, lib.c_mem_counts.restype = [u64p], None
    lib.c_elem_size.argtypes, lib.c_elem_size.restype = [C.c_int], C.c_uint64
    lib.c_group_new.argtypes, lib.c_group_new.restype = [], vp
    lib.c_group_free.argtypes, lib.c_group_free.restype = [vp], None
    lib.c_block_ensure.argtypes, lib.c_block_ensure.restype = [vp, C.c_int, C.c_uint64], C.c_int
    lib.c_group_ensure.argtypes, lib.c_group_ensure.restype = [vp, u64p, C.POINTER(C.c_int)], C.c_int
    lib.c_group_holds.argtypes, lib.c_group_holds.restype = [vp, u64p], C.c_int
    lib.c_group_state.argtypes, lib.c_group_state.restype = [vp, u64p, u64p], None
    lib.c_move_case.argtypes, lib.c_move_case.restype = [u64p], None
    _lib = lib
    return lib


class Mem:
    """the allocator's counters since the last reset"""

    def __init__(self, fail_at=-1):
        probe().c_mem_reset(fail_at)

    @property
    def counts(self):
        out = (C.c_uint64 * 4)()
        probe().c_mem_counts(out)
        return dict(zip(("calls", "allocs", "frees", "last_bytes"), out))


class Group:
    def __init__(self):
        self.g = probe().c_group_new()

    def close(self):
        probe().c_group_free(self.g)
        self.g = None

    def ensure_one(self, i, n):
        return probe().c_block_ensure(self.g, i, n)

    def ensure(self, counts):
        """-> (ok, moved)"""
        moved = C.c_int(-1)
        ok = probe().c_group_ensure(self.g, (C.c_uint64 * K)(*counts), C.byref(moved))
        return bool(ok), bool(moved.value)

    def holds(self, counts):
        return bool(probe().c_group_holds(self.g, (C.c_uint64 * K)(*counts)))

    @property
    def state(self):
        """-> (pointers, counts)"""
        ptr, cnt = (C.c_uint64 * K)(), (C.c_uint64 * K)()
        probe().c_group_state(self.g, ptr, cnt)
        return list(ptr), list(cnt)


@pytest.fixture
def group():
    g = Group()
    yield g
    if g.g is not None:
        g.close()


EMPTY = ([0] * K, [0] * K)


# ── 1. ensure ──────────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("i", range(K))
def test_ensure_allocates_keeps_moves_and_is_empty_after_a_failed_regrow(group, i):
    size = probe().c_elem_size(i)
    mem = Mem()
    assert group.ensure_one(i, 10) == MOVED  # empty: allocates
    p0, c0 = group.state[0][i], group.state[1][i]
    assert p0 != 0 and c0 == 10 and mem.counts == dict(calls=1, allocs=1, frees=0, last_bytes=10 * size)
    for n in (10, 9, 1, 0):  # smaller or equal: nothing happens
        assert group.ensure_one(i, n) == KEPT
        assert (group.state[0][i], group.state[1][i]) == (p0, 10)
    assert mem.counts["calls"] == 1 and mem.counts["frees"] == 0
    assert group.ensure_one(i, 11) == MOVED  # larger: frees, then allocates
    assert group.state[1][i] == 11 and group.state[0][i] != 0
    assert mem.counts == dict(calls=2, allocs=2, frees=1, last_bytes=11 * size)
    others = [j for j in range(K) if j != i]
    assert all(group.state[0][j] == 0 and group.state[1][j] == 0 for j in others)
    mem = Mem(fail_at=0)
    assert group.ensure_one(i, 12) == FAILED  # never the old pointer, never a count it does not have
    assert group.state == EMPTY and mem.counts == dict(calls=1, allocs=0, frees=1, last_bytes=0)
    mem = Mem()
    assert group.ensure_one(i, 12) == MOVED and group.state[1][i] == 12  # ... and usable again
    group.close()
    assert mem.counts["allocs"] == 1 and mem.counts["frees"] == 1


def test_ensure_zero_on_an_empty_block_allocates_nothing(group):
    mem = Mem()
    assert all(group.ensure_one(i, 0) == KEPT for i in range(K))
    assert group.state == EMPTY and mem.counts["calls"] == 0


# ── 2. the group ───────────────────────────────────────────────────────────────────────────────────────────────────────

COUNTS = [5, 1, 9, 2, 3]


@pytest.mark.parametrize("j", range(K))
def test_group_is_all_or_nothing_when_the_jth_allocation_fails(group, j):
    mem = Mem(fail_at=j)
    assert group.ensure(COUNTS) == (False, True)
    assert group.state == EMPTY  # all five, the j that were allocated before the failure too
    assert mem.counts["allocs"] == j and mem.counts["frees"] == j and mem.counts["calls"] == j + 1
    assert not group.holds(COUNTS)
    mem = Mem()  # a later call with memory available succeeds
    assert group.ensure(COUNTS) == (True, True)
    ptr, cnt = group.state
    assert cnt == COUNTS and all(ptr) and len(set(ptr)) == K and group.holds(COUNTS)
    assert mem.counts["allocs"] == K and mem.counts["frees"] == 0
    group.close()
    assert mem.counts["frees"] == K


def test_group_allocates_only_the_members_that_do_not_hold_enough(group):
    mem = Mem()
    for i in (0, 1, 2):  # the first members hold enough already (one of them more than enough)
        assert group.ensure_one(i, COUNTS[i] + (i == 1)) == MOVED
    before = group.state
    assert mem.counts["allocs"] == 3
    assert group.ensure(COUNTS) == (True, True)
    ptr, cnt = group.state
    assert ptr[:3] == before[0][:3] and cnt == [5, 2, 9, 2, 3] and all(ptr)
    assert mem.counts["allocs"] == 5 and mem.counts["frees"] == 0
    assert group.ensure(COUNTS) == (True, False) and group.state == (ptr, cnt)  # nothing to do: nothing moved
    assert mem.counts["calls"] == 5


def test_a_failed_group_empties_the_members_that_held_enough_too(group):
    Mem()
    assert group.ensure(COUNTS) == (True, True)
    grown = COUNTS[:4] + [COUNTS[4] + 1]
    mem = Mem(fail_at=0)
    assert group.ensure(grown) == (False, True)  # ("moved": no pointer is what it was)
    assert group.state == EMPTY and mem.counts["allocs"] == 0 and mem.counts["frees"] == K


# ── 3. move and destruction ────────────────────────────────────────────────────────────────────────────────────────────

def test_move_leaves_the_source_empty_and_destruction_frees_once():
    out = (C.c_uint64 * 10)()
    probe().c_move_case(out)
    p = out[0]
    assert p != 0
    assert (out[1], out[2]) == (0, 0) and (out[3], out[4]) == (p, 7) and out[5] == 0  # move construction: no free, no copy
    assert (out[6], out[7]) == (p, 7) and out[8] == 1  # move assignment: the target's old memory goes, the source is empty
    assert out[9] == 2  # two allocations, two frees: nothing freed twice, nothing kept


def test_destruction_frees_every_block_exactly_once():
    mem = Mem()
    g = Group()
    assert g.ensure(COUNTS) == (True, True)
    g.close()
    assert mem.counts["allocs"] == K and mem.counts["frees"] == K
    g = Group()
    g.close()  # empty blocks free nothing
    assert mem.counts["frees"] == K


# ── 4. overflow ────────────────────────────────────────────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("i", range(1, K))
def test_a_count_whose_bytes_overflow_size_t_is_refused_without_an_allocator_call(group, i):
    size = probe().c_elem_size(i)
    mem = Mem()
    for n in (SIZE_MAX // size + 1, SIZE_MAX):
        assert group.ensure_one(i, n) == FAILED
        assert group.state == EMPTY and mem.counts["calls"] == 0
    counts = list(COUNTS)
    counts[i] = SIZE_MAX // size + 1
    assert group.ensure(counts) == (False, True)  # ... inside a group: the members before it are given back
    assert group.state == EMPTY and mem.counts["calls"] == i and mem.counts["frees"] == i


# ── 5. the probe's own program under the sanitizers ────────────────────────────────────────────────────────────────────

def test_probe_program_under_asan_ubsan():
    exe = BUILD / "dev_block_probe_san"
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DDEV_BLOCK_PROBE_MAIN", "-o", str(exe),
                    str(SRCS[0])], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "dev_block_probe ok" in r.stdout, r.stdout + r.stderr
