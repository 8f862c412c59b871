// qkv_colocate.h — which block id plays which role in the fused q / k / v + decode attention launch of n-on-lanes weights
// (qmatvec.hip: qkv_attn_kernel). Plain C++: the kernel, its launcher and the host probe (tests/cpp/qkv_colocate_probe.cpp)
// include it alike.
//
// The launch has n_mv projection column groups (16 outputs each: q, then k, then v) and n_heads x n_sp attention workgroups. The
// hand-off between them is head-local: a head needs its own d_head / 16 q column groups and the d_head / 16 k and v column
// groups of its kv group. Blocks b and b + 8 are observed to share an XCD, so `b % 8` is a LABEL of blocks that share one
// (which XCD is not known, and nothing but speed may depend on it: the hand-off itself is placement-independent, handoff_gen.h).
// The map below gives kv group j the label j % 8 and puts on that label
//   - first (lowest ids: dispatched first) the group's projection column groups: (n_heads / n_kv) d_head / 16 of q, d_head / 16 of k
//     and of v — all groups of the label one after the other,
//   - then split 0 of the group's heads (the split that is live at every position),
// and deals the ids that are left, label by label, to the splits >= 1 in head-major order. The grid is not padded: where some
// label has fewer ids than its groups need, the map is the identity (`on` == 0) and the launch is what it was.
//
// Roles: r < n_mv is projection column group r of the launch (q | k | v order); otherwise r - n_mv = split * n_heads + record
// is an attention workgroup (head-major, as without the map). The map assumes record i belongs to kv group i / (n_heads / n_kv);
// the planner switches it off where the records are not in that order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZGML_COLOCATE_HD __host__ __device__
#else
#define ZGML_COLOCATE_HD
#endif

namespace zgml {

struct QkvColocate {
    uint32_t on;     // 0: identity
    uint32_t n_kv;   // kv groups (<= 255)
    uint32_t pk;     // projection column groups of k (= of v) per kv group: d_head / 16 (<= 255)
    uint32_t hpg;    // heads per kv group (<= 32767): its split-0 attention workgroups, and pq = hpg * pk column groups of q
};
// ... as ONE dword, so that it can travel with the kernel's preloaded leading arguments (0 = identity)
ZGML_COLOCATE_HD inline uint32_t qkv_colocate_pack(const QkvColocate& c) { return c.on ? 0x80000000u | (c.hpg << 16) | (c.pk << 8) | c.n_kv : 0u; }
ZGML_COLOCATE_HD inline QkvColocate qkv_colocate_unpack(uint32_t w) { return QkvColocate{w >> 31, w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0x7FFFu}; }

ZGML_COLOCATE_HD inline uint32_t qkv_colocate_groups_on(uint32_t label, uint32_t n_kv) { return label < n_kv ? (n_kv - label + 7) >> 3 : 0; }
ZGML_COLOCATE_HD inline uint32_t qkv_colocate_ids_on(uint32_t label, uint32_t grid) { return grid > label ? (grid - label + 7) >> 3 : 0; }

// The map for a launch of these dimensions (all-zero = identity where the groups do not fit their labels).
inline QkvColocate qkv_colocate_plan(uint32_t n_heads, uint32_t n_kv, uint32_t d_head, uint32_t n_sp) {
    QkvColocate c{};
    if (!n_heads || !n_kv || n_heads % n_kv || !d_head || d_head % 16 || !n_sp) return c;
    const uint32_t hpg = n_heads / n_kv, pk = d_head / 16, per_group = (hpg + 2) * pk + hpg;
    if (n_kv > 255 || pk > 255 || hpg > 32767) return c;
    const unsigned long long grid = (unsigned long long)n_kv * (hpg + 2) * pk + (unsigned long long)n_heads * n_sp;
    if (grid >= (1ull << 31)) return c;
    for (uint32_t l = 0; l < 8; l++)
        if ((unsigned long long)qkv_colocate_groups_on(l, n_kv) * per_group > qkv_colocate_ids_on(l, (uint32_t)grid)) return c;
    c.on = 1, c.n_kv = n_kv, c.pk = pk, c.hpg = hpg;
    return c;
}

// The role of block `b` of a grid of n_mv + n_heads * n_sp blocks. A bijection on [0, grid) for every `c` that
// qkv_colocate_plan returns for these dimensions. Scalar arithmetic on `c`, `b` and n_mv alone for the projection's roles (the
// kernel runs it in front of its first load, from preloaded arguments); n_heads and n_sp are read for splits >= 1 only.
ZGML_COLOCATE_HD inline uint32_t qkv_colocate_role(const QkvColocate& c, uint32_t b, uint32_t n_mv, uint32_t n_heads, uint32_t n_sp) {
    if (!c.on) return b;
    const uint32_t label = b & 7, pq = c.hpg * c.pk, p = pq + 2 * c.pk, groups = qkv_colocate_groups_on(label, c.n_kv);
    const uint32_t n_pro = groups * p, n_con = groups * c.hpg;
    uint32_t t = b >> 3, j = label; // (kv group j = label + 8 s: the s-th group of this label; seldom more than one)
    if (t < n_pro) { // a projection column group of kv group j
        while (t >= p) t -= p, j += 8;
        if (t < pq) return j * pq + t;
        if (t < pq + c.pk) return c.n_kv * pq + j * c.pk + (t - pq);
        return c.n_kv * (pq + c.pk) + j * c.pk + (t - pq - c.pk);
    }
    t -= n_pro;
    if (t < n_con) { // split 0 of a head of kv group j
        while (t >= c.hpg) t -= c.hpg, j += 8;
        return n_mv + j * c.hpg + t;
    }
    // the ids no group needs, label by label: splits >= 1, head-major
    const uint32_t grid = n_mv + n_heads * n_sp;
    uint32_t rank = t - n_con;
    for (uint32_t l = 0; l < 7; l++)
        if (l < label) rank += qkv_colocate_ids_on(l, grid) - qkv_colocate_groups_on(l, c.n_kv) * (p + c.hpg);
    return n_mv + n_heads + rank;
}

} // namespace zgml
