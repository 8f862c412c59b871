// qkv_colocate_probe — walks the block map of the fused q / k / v + decode attention launch (zgml_amd/csrc/qkv_colocate.h) on the
// CPU for tests/test_qkv_colocate_host.py (built with -fsanitize=address,undefined by the test). For every case
// (n_heads, n_kv, d_head, n_sp) of the table, or of the command line, it evaluates the role of every block id and prints one line:
//   fits       every label b % 8 has at least as many ids as the kv groups dealt to it need (counted here, id by id)
//   on         the map the planner function returns is not the identity
//   bijection  every role of [0, grid) is taken exactly once
//   colocated  (on) every projection column group of a kv group and split 0 of each of its heads carry one label
//   ordered    (on) on every label the projection's ids are all lower than the ids of the attention's workgroups
//   identity   role(b) == b for every b
//   packed     the map survives the one-dword form the kernel receives
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../zgml_amd/csrc/qkv_colocate.h"

using namespace zgml;

struct Case {
    uint32_t n_heads, n_kv, d_head, n_sp;
};

static bool run(const Case& k) {
    const uint32_t hpg = k.n_heads / k.n_kv, pk = k.d_head / 16, pq = hpg * pk;
    const uint32_t n_mv = (k.n_heads + 2 * k.n_kv) * pk, grid = n_mv + k.n_heads * k.n_sp;
    // does every label hold its groups? counted id by id, not by the header's formulas
    std::vector<uint32_t> ids(8, 0), need(8, 0);
    for (uint32_t b = 0; b < grid; b++) ids[b % 8]++;
    for (uint32_t j = 0; j < k.n_kv; j++) need[j % 8] += pq + 2 * pk + hpg;
    bool fits = true;
    for (int l = 0; l < 8; l++) fits = fits && need[l] <= ids[l];

    const QkvColocate c = qkv_colocate_plan(k.n_heads, k.n_kv, k.d_head, k.n_sp);
    const QkvColocate u = qkv_colocate_unpack(qkv_colocate_pack(c));
    const bool packed = u.on == c.on && u.n_kv == c.n_kv && u.pk == c.pk && u.hpg == c.hpg;

    std::vector<uint32_t> block_of(grid, UINT32_MAX); // role -> block id
    bool bijection = true, identity = true;
    for (uint32_t b = 0; b < grid; b++) {
        const uint32_t r = qkv_colocate_role(u, b, n_mv, k.n_heads, k.n_sp);
        identity = identity && r == b;
        if (r >= grid || block_of[r] != UINT32_MAX) {
            bijection = false;
            continue;
        }
        block_of[r] = b;
    }
    bool colocated = true, ordered = true;
    if (bijection && c.on) {
        std::vector<uint32_t> hi_pro(8, 0), lo_con(8, UINT32_MAX); // per label: the projection's highest id, the attention's lowest
        for (uint32_t j = 0; j < k.n_kv; j++) {
            const uint32_t label = block_of[j * pq] % 8;
            auto producer = [&](uint32_t cg) {
                colocated = colocated && block_of[cg] % 8 == label;
                if (block_of[cg] > hi_pro[block_of[cg] % 8]) hi_pro[block_of[cg] % 8] = block_of[cg];
            };
            for (uint32_t i = 0; i < pq; i++) producer(j * pq + i);
            for (uint32_t i = 0; i < pk; i++) producer(k.n_kv * pq + j * pk + i), producer(k.n_kv * (pq + pk) + j * pk + i);
            for (uint32_t h = j * hpg; h < (j + 1) * hpg; h++) { // split 0 of head h: attention workgroup h (head-major)
                const uint32_t b = block_of[n_mv + h];
                colocated = colocated && b % 8 == label;
            }
        }
        for (uint32_t r = n_mv; r < grid; r++) // (every attention workgroup of the label counts, not split 0 alone)
            if (block_of[r] < lo_con[block_of[r] % 8]) lo_con[block_of[r] % 8] = block_of[r];
        for (int l = 0; l < 8; l++) ordered = ordered && (lo_con[l] == UINT32_MAX || hi_pro[l] < lo_con[l]);
    }
    printf("case=%u,%u,%u,%u grid=%u fits=%d on=%d bijection=%d colocated=%d ordered=%d identity=%d packed=%d\n", k.n_heads, k.n_kv, k.d_head, k.n_sp, grid,
           fits ? 1 : 0, c.on ? 1 : 0, bijection ? 1 : 0, colocated ? 1 : 0, ordered ? 1 : 0, identity ? 1 : 0, packed ? 1 : 0);
    return bijection && packed && (c.on != 0) == fits && (c.on ? colocated && ordered : identity);
}

int main(int argc, char** argv) {
    std::vector<Case> cases = {{9, 3, 64, 16}, {9, 3, 64, 1}, {32, 32, 128, 2}, {32, 8, 128, 4}, {4, 1, 64, 16}, {12, 12, 64, 8}, {64, 8, 128, 1}};
    if (argc > 1) { // n_heads n_kv d_head n_sp, repeated
        cases.clear();
        for (int i = 1; i + 3 < argc; i += 4)
            cases.push_back({(uint32_t)atoi(argv[i]), (uint32_t)atoi(argv[i + 1]), (uint32_t)atoi(argv[i + 2]), (uint32_t)atoi(argv[i + 3])});
    }
    bool ok = true;
    for (const Case& k : cases) {
        if (!k.n_heads || !k.n_kv || k.n_heads % k.n_kv || !k.d_head || k.d_head % 16 || !k.n_sp) {
            printf("case=%u,%u,%u,%u not a launch\n", k.n_heads, k.n_kv, k.d_head, k.n_sp);
            ok = false;
            continue;
        }
        ok = run(k) && ok;
    }
    printf("ok=%d\n", ok ? 1 : 0);
    return ok ? 0 : 1;
}
