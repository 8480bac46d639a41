// hgx_not_dev.h -- the device side of the negation program (include/hgx_not.h), shared by the two stages that
// evaluate it on a link row: the filter over clause hits (hgx_not.hip) and the type-index scan (hgx_scan.hip).
// One definition of the candidate link, of the leaves' raw satisfies and of the walk over a clause's
// negations; the two kernels differ only in where the row comes from.
#pragma once

#include "hgx_internal.h"

namespace hgx {

// first i in [0, n) with a[i] > v (n when none)
__device__ __forceinline__ int64_t upper_bound_off(const int64_t* __restrict__ a, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void wave_add(u64* p, u64 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(p, v);
}

// The candidate link of one lane: its target row, the first 8 targets in registers.
struct Link {
    const int32_t* tg;
    int32_t n;
    int32_t r[8];
};

// f(position, target) for the targets in layout order until f returns true
template <class F>
__device__ __forceinline__ void each_target(const Link& L, F f) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= L.n) return;
        if (f(k, L.r[k])) return;
    }
    for (int32_t i = 8; i < L.n; ++i)
        if (f(i, L.tg[i])) return;
}

// The raw satisfies of one leaf (include/hgx_not.h) with the operands op[0, m).  type == INT32_MIN: not read
// yet (link_type[row] on the first type literal); a caller that knows the type hands it over and link_type is
// never touched.
__device__ __forceinline__ bool leaf_satisfies(int32_t kind, const int32_t* __restrict__ op, int32_t m, const Link& L,
                                               const int32_t* __restrict__ link_type, int64_t row, int32_t& type,
                                               u64& types_read) {
    switch (kind) {
    case HGX_NOT_TYPE: {
        if (type == INT32_MIN) {
            type = link_type[row];
            ++types_read;
        }
        for (int32_t i = 0; i < m; ++i)
            if (op[i] == type) return true;
        return false;
    }
    case HGX_NOT_INCIDENT: {
        const int32_t x = op[0];
        bool found = false;
        each_target(L, [&](int32_t, int32_t t) { return found = t == x; });
        return found;
    }
    case HGX_NOT_POSITIONED: {
        const int32_t x = op[0], comp = op[3];
        int64_t lb = op[1], ub = op[2];
        if (ub < 0) ub += L.n;
        if (lb < 0) lb += L.n;
        if (lb > ub || lb < 0 || ub < 0 || lb >= L.n || ub >= L.n) return false;
        bool found = false;
        each_target(L, [&](int32_t i, int32_t t) { return found = t == x && ((i >= lb && i <= ub) != (comp != 0)); });
        return found;
    }
    case HGX_NOT_ORDERED: {
        int32_t j = 0;
        each_target(L, [&](int32_t, int32_t t) {
            if (j >= m) return true;
            const int32_t p = op[j];
            if (p == HGX_ANY_HANDLE || p == t) ++j;
            return false;
        });
        return j == m;
    }
    case HGX_NOT_LINK: {
        int32_t count = 0;
        each_target(L, [&](int32_t, int32_t t) {
            for (int32_t k = 0; k < m; ++k)
                if (op[k] == t) {
                    ++count;
                    break;
                }
            return false;
        });
        return count == m;
    }
    default:   // HGX_NOT_ARITY (the host refuses every other kind)
        return L.n == op[0];
    }
}

// The satisfies of one leaf on a NODE atom of the type `type` (include/hgx_atoms.h): arity(k) holds iff k == 0
// (ArityCondition.java:54-55), a type leaf compares the atom's type, every leaf that reads targets is false --
// an empty orderedLink() / link() included, which holds on a link without targets.
__device__ __forceinline__ bool node_leaf_satisfies(int32_t kind, const int32_t* __restrict__ op, int32_t m, int32_t type) {
    if (kind == HGX_NOT_TYPE) {
        for (int32_t i = 0; i < m; ++i)
            if (op[i] == type) return true;
        return false;
    }
    return kind == HGX_NOT_ARITY && op[0] == 0;
}

// The negations [g0, g1) of one clause on the link L: true iff no negated tree holds (a negated tree holds
// when one of its terms has every literal holding).  NODE: the atom is a node of the type `type` (L is not read).
template <bool NODE = false>
__device__ __forceinline__ bool negations_keep(const NotDev& prog, int64_t g0, int64_t g1, const Link& L,
                                               const int32_t* __restrict__ link_type, int64_t row, int32_t& type,
                                               u64& types_read) {
    bool keep = true;
    for (int64_t g = g0; g < g1 && keep; ++g) {
        bool p = false;
        for (int64_t t = prog.term_off[g], t1 = prog.term_off[g + 1]; t < t1 && !p; ++t) {
            bool all = true;
            for (int64_t l = prog.lit_off[t], l1 = prog.lit_off[t + 1]; l < l1 && all; ++l) {
                const int4 rec = prog.lit[l];
                const bool s = NODE ? node_leaf_satisfies(rec.x, prog.ops + rec.z, rec.w - rec.z, type)
                                    : leaf_satisfies(rec.x, prog.ops + rec.z, rec.w - rec.z, L, link_type, row, type,
                                                     types_read);
                all = s == (rec.y != 0);
            }
            p = all;
        }
        keep = !p;
    }
    return keep;
}

}  // namespace hgx
