// dev_block_probe.cpp — zgml_amd/csrc/dev_block.h (the owner of a device block and the all-or-nothing group ensure) over a
// counting malloc / free that fails at a chosen call, behind a C ABI for the CPU tests (tests/test_dev_block_host.py). The
// header is the rule; added here is only a group of five blocks of mixed element sizes and the counters.
// Build: g++ -O1 -std=c++17 -Wall -Werror -shared -fPIC. With -DDEV_BLOCK_PROBE_MAIN the file is a stand-alone program that
// walks the same cases (built with -fsanitize=address,undefined by the tests: the sanitizer's leak and double-free checks
// then see what the header does with real memory).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../zgml_amd/csrc/dev_block.h"

using namespace zgml;

namespace {

struct CountingMem {
    static inline int64_t calls = 0, allocs = 0, frees = 0, fail_at = -1; // fail_at: the index of the alloc call that fails (-1: none)
    static inline uint64_t last_bytes = 0;
    static void* alloc(size_t bytes) {
        if (calls++ == fail_at) return nullptr;
        allocs++, last_bytes = bytes;
        return malloc(bytes ? bytes : 1);
    }
    static void free(void* p) {
        frees++;
        ::free(p);
    }
};
template <class T>
using Block = dev_block<T, CountingMem>;

struct Wide {
    uint64_t w[3]; // 24 bytes: an element size that is no power of two
};

constexpr int kBlocks = 5;
struct Group {
    Block<uint8_t> a;
    Block<uint16_t> b;
    Block<uint32_t> c;
    Block<uint64_t> d;
    Block<Wide> e;
};
constexpr size_t kElem[kBlocks] = {1, 2, 4, 8, sizeof(Wide)};

int code(DevEnsure e) { return e == DevEnsure::Failed ? 0 : e == DevEnsure::Kept ? 1 : 2; }

} // namespace

extern "C" {

// the counters back to 0; the fail_at-th alloc call from now on fails (-1: none)
void c_mem_reset(int64_t fail_at) { CountingMem::calls = CountingMem::allocs = CountingMem::frees = 0, CountingMem::fail_at = fail_at, CountingMem::last_bytes = 0; }
// out: alloc calls, allocations made, frees made, bytes of the last allocation
void c_mem_counts(uint64_t* out) { out[0] = CountingMem::calls, out[1] = CountingMem::allocs, out[2] = CountingMem::frees, out[3] = CountingMem::last_bytes; }

uint64_t c_elem_size(int i) { return kElem[i]; }
void* c_group_new() { return new Group(); }
void c_group_free(void* g) { delete (Group*)g; }

// block i alone: 0 failed, 1 kept, 2 moved
int c_block_ensure(void* gv, int i, uint64_t n) {
    Group* g = (Group*)gv;
    return code(i == 0 ? g->a.ensure(n) : i == 1 ? g->b.ensure(n) : i == 2 ? g->c.ensure(n) : i == 3 ? g->d.ensure(n) : g->e.ensure(n));
}

// the five as one group; *moved as dev_ensure reports it
int c_group_ensure(void* gv, const uint64_t* n, int* moved) {
    Group* g = (Group*)gv;
    bool m = false;
    const bool ok = dev_ensure(&m, g->a, n[0], g->b, n[1], g->c, n[2], g->d, n[3], g->e, n[4]);
    *moved = m;
    return ok;
}
int c_group_holds(void* gv, const uint64_t* n) {
    const Group* g = (const Group*)gv;
    return dev_holds(g->a, n[0], g->b, n[1], g->c, n[2], g->d, n[3], g->e, n[4]);
}

// pointer (through the implicit conversion a launch argument takes) and count of every block
void c_group_state(void* gv, uint64_t* ptr, uint64_t* count) {
    const Group* g = (const Group*)gv;
    const void* p[kBlocks] = {(uint8_t*)g->a, (uint16_t*)g->b, (uint32_t*)g->c, (uint64_t*)g->d, (Wide*)g->e};
    const size_t c[kBlocks] = {g->a.count(), g->b.count(), g->c.count(), g->d.count(), g->e.count()};
    for (int i = 0; i < kBlocks; i++) ptr[i] = (uint64_t)(uintptr_t)p[i], count[i] = c[i];
}

// move construction and move assignment; out: [0] the pointer allocated, [1, 2] the source's pointer and count after the move
// construction, [3, 4] the target's, [5] frees so far, [6, 7] the target of a move assignment over a block that held memory,
// [8] frees after it (its old memory: one), [9] frees after every block has gone (two allocations, two frees)
void c_move_case(uint64_t* out) {
    c_mem_reset(-1);
    {
        Block<uint32_t> x;
        x.ensure(7);
        out[0] = (uint64_t)(uintptr_t)x.get();
        Block<uint32_t> y(std::move(x));
        out[1] = (uint64_t)(uintptr_t)x.get(), out[2] = x.count(); // NOLINT: the moved-from state is the point
        out[3] = (uint64_t)(uintptr_t)y.get(), out[4] = y.count();
        out[5] = CountingMem::frees;
        Block<uint32_t> z;
        z.ensure(3);
        z = std::move(y);
        out[6] = (uint64_t)(uintptr_t)z.get(), out[7] = z.count() + (y.get() ? 1000 : 0) + (y.count() ? 1000 : 0); // NOLINT
        out[8] = CountingMem::frees;
    }
    out[9] = CountingMem::frees;
}

} // extern "C"

#ifdef DEV_BLOCK_PROBE_MAIN
int main() {
    uint64_t ptr[kBlocks], cnt[kBlocks], m[4];
    int moved = 0;
    // ensure: empty -> allocated; smaller or equal -> kept; larger -> moved; a failed regrow -> empty
    c_mem_reset(-1);
    void* g = c_group_new();
    if (c_block_ensure(g, 2, 10) != 2 || c_block_ensure(g, 2, 10) != 1 || c_block_ensure(g, 2, 3) != 1 || c_block_ensure(g, 2, 11) != 2) return 1;
    c_mem_counts(m);
    if (m[0] != 2 || m[1] != 2 || m[2] != 1 || m[3] != 44) return 2;
    c_mem_reset(0);
    if (c_block_ensure(g, 2, 12) != 0) return 3;
    c_group_state(g, ptr, cnt);
    c_mem_counts(m);
    if (ptr[2] || cnt[2] || m[1] != 0 || m[2] != 1) return 4;
    // overflow: refused without a call
    c_mem_reset(-1);
    if (c_block_ensure(g, 4, SIZE_MAX / sizeof(Wide) + 1) != 0 || c_block_ensure(g, 3, (uint64_t)1 << 61) != 0) return 5;
    c_mem_counts(m);
    if (m[0] != 0) return 6;
    c_group_free(g);
    // the group: fail the j-th allocation -> all empty, allocations == frees; the retry fills all five
    const uint64_t n[kBlocks] = {5, 1, 9, 2, 3}, more[kBlocks] = {5, 1, 10, 2, 4};
    for (int j = 0; j < kBlocks; j++) {
        g = c_group_new();
        c_mem_reset(j);
        if (c_group_ensure(g, n, &moved) || !moved) return 10 + j;
        c_group_state(g, ptr, cnt);
        c_mem_counts(m);
        for (int i = 0; i < kBlocks; i++)
            if (ptr[i] || cnt[i]) return 20 + j;
        if (m[1] != (uint64_t)j || m[2] != (uint64_t)j) return 30 + j;
        c_mem_reset(-1);
        if (!c_group_ensure(g, n, &moved) || !moved || !c_group_holds(g, n)) return 40 + j;
        c_group_state(g, ptr, cnt);
        for (int i = 0; i < kBlocks; i++) {
            if (!ptr[i] || cnt[i] != n[i]) return 50 + j;
            for (size_t k = 0; k < n[i] * kElem[i]; k++) ((volatile uint8_t*)(uintptr_t)ptr[i])[k] = (uint8_t)k; // (every byte it owns)
        }
        // members that hold enough stay; only the rest is allocated
        c_mem_reset(-1);
        if (!c_group_ensure(g, n, &moved) || moved) return 60 + j;
        if (!c_group_ensure(g, more, &moved) || !moved) return 70 + j;
        c_mem_counts(m);
        if (m[0] != 2 || m[2] != 2) return 80 + j;
        // a failure in a group that held memory empties the members that held enough too
        c_mem_reset(0);
        const uint64_t most[kBlocks] = {5, 1, 10, 2, 5};
        if (c_group_ensure(g, most, &moved) || !moved) return 90 + j;
        c_group_state(g, ptr, cnt);
        for (int i = 0; i < kBlocks; i++)
            if (ptr[i] || cnt[i]) return 100 + j;
        c_group_free(g);
    }
    uint64_t mv[10];
    c_move_case(mv);
    if (!mv[0] || mv[1] || mv[2] || mv[3] != mv[0] || mv[4] != 7 || mv[5] != 0 || mv[6] != mv[0] || mv[7] != 7 || mv[8] != 1 || mv[9] != 2) return 7;
    // destruction frees exactly once
    c_mem_reset(-1);
    g = c_group_new();
    if (!c_group_ensure(g, n, &moved)) return 8;
    c_group_free(g);
    c_mem_counts(m);
    if (m[1] != kBlocks || m[2] != kBlocks) return 9;
    printf("dev_block_probe ok\n");
    return 0;
}
#endif
