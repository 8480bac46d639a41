// hgx_join.hip -- pattern hits projected to a link target and the projections intersected on the device
// (hgx_pattern_batch_join, include/hgx_join.h).
//
// Replaces ResultMapQuery over LinkProjectionMapping (C/query/cond2qry/ToQueryMap.java:409-427,
// C/query/impl/LinkProjectionMapping.java:33-36) -- hg.apply(hg.targetAt(graph, p), cond) -- and the And of
// such conditions, the reference's pattern test (TC/query/PatternTests.java:20-61).  The inner conditions are
// the parts of the batch: each part is one query of a DNF batch, evaluated by the clause stage, the filter, the
// scan and the union (hgx_query.hip, hgx_not.hip, hgx_scan.hip, hgx_union.hip), which leaves part s's link
// atoms in device memory as uids[uoff[s], uoff[s+1]), ascending; join query j owns the parts
// [part_off[j], part_off[j+1]).
//
// GPU formulation, deterministic, no atomic decides an order:
//   hgx_join_key   -- a lane per union hit e: its part s (binary search of uoff), the link's row (binary search
//        of the ascending link_atom, as the negation filter finds it), and the 64-bit key (s << 32) | v with
//        v = targets(L)[p], L itself for HGX_JOIN_SELF, 0xFFFFFFFF (above every atom id) for a link too short.
//        Lanes past the hit total write a pad key whose part is n_parts: the sort is sized from the workspace
//        capacity (the hit total is known on the device only) and the pads sort behind every hit;
//   the sort       -- rocprim::radix_sort_keys over the low 32 + bits(n_parts) bits.  The part is the high
//        field, so part s still owns [uoff[s], uoff[s+1]) of the sorted keys, now ascending by value;
//   hgx_join_keep  -- a lane per sorted key.  The driver of join query j is its part with the fewest hits
//        (ties: the lowest index).  A key is kept iff it belongs to its query's driver, is no sentinel, differs
//        from its predecessor and a binary search finds its value in the segment of every other part of j.  With
//        atom predicates (hgx_pattern_batch_atoms, include/hgx_atoms.h) the FILTER instantiation tests the value's
//        bit in its query's bitmap after the driver test and before those searches;
//   the scan       -- pre = exclusive prefix sum of the keep flags (rocPRIM);
//   hgx_join_place -- a kept key's value goes to pre[i]; qoff[j] = pre[uoff[part_off[j]]]; lane 0 publishes
//        the totals and the counters into the mapped result area.
// Every kernel reads the hit total and the overflow flag of the clause stage from device memory and does
// nothing after an overflow: no host round trip sits between the union and the join.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hgx_not_dev.h"

namespace hgx {

namespace {

constexpr u64 kMissing = 0xFFFFFFFFull;   // the value of a link too short for the position

// first i in [b, e) with a[i] >= k (e when none)
__device__ __forceinline__ int64_t lower_bound_key(const u64* __restrict__ a, int64_t b, int64_t e, u64 k, u64& probes) {
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        ++probes;
        if (a[mid] < k) b = mid + 1;
        else e = mid;
    }
    return b;
}

__global__ void __launch_bounds__(256) hgx_join_key(JoinArgs a) {
    if (a.stat[2]) return;   // the clause stage overflowed its workspace: the host grows it and runs again
    const int64_t H = a.uoff[a.n_parts];
    const u64 pad = ((u64)a.n_parts << 32) | kMissing;
    u64 probes = 0, targets_read = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.cap; e += (int64_t)gridDim.x * blockDim.x) {
        if (e >= H) {
            a.key[e] = pad;
            continue;
        }
        int64_t lo = 0, hi = (int64_t)a.n_parts + 1;   // the part: first offset > e, minus one
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            ++probes;
            if (a.uoff[mid] <= e) lo = mid + 1;
            else hi = mid;
        }
        const int64_t s = lo - 1;
        const int32_t x = a.uids[e], p = a.part_pos[s];
        u64 v = (u64)(uint32_t)x;
        if (p >= 0) {
            int64_t row = 0, rh = a.M;   // the link's row: first row with link_atom >= x
            while (row < rh) {
                const int64_t mid = (row + rh) >> 1;
                ++probes;
                if (a.link_atom[mid] < x) row = mid + 1;
                else rh = mid;
            }
            v = kMissing;
            if (row < a.M && a.link_atom[row] == x) {   // (a hit is a link atom)
                const int64_t b = a.tgt_off[row];
                if ((int64_t)p < a.tgt_off[row + 1] - b) {
                    v = (u64)(uint32_t)a.tgt_idx[b + p];
                    ++targets_read;
                }
            }
        }
        a.key[e] = ((u64)s << 32) | v;
    }
    wave_add(a.ctr + 3, probes);
    wave_add(a.ctr + 5, targets_read);
}

// FILTER (hgx_pattern_batch_atoms with predicates): a key that is the first of its value in its query's driver
// part tests its bit in the query's bitmap (one 8-byte load) before the probes of the other parts.  A batch
// without predicates runs the instantiation without the test.
template <bool FILTER>
__global__ void __launch_bounds__(256) hgx_join_keep(JoinArgs a) {
    if (a.stat[2]) return;
    const int64_t H = a.uoff[a.n_parts];
    const u64* __restrict__ ks = a.key_sorted;
    u64 probes = 0, distinct = 0, tested = 0, rejected = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < H; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = ks[i];
        const int64_t s = (int64_t)(k >> 32);
        const u64 v = k & kMissing;
        const int64_t b = a.uoff[s];
        const bool first = v != kMissing && (i == b || ks[i - 1] != k);   // a distinct value of its part
        if (first) ++distinct;
        bool keep = first;
        if (keep) {
            const int64_t j = upper_bound_off(a.part_off, (int64_t)a.n_queries + 1, s) - 1;
            const int64_t s0 = a.part_off[j], s1 = a.part_off[j + 1];
            int64_t drv = s0, best = a.uoff[s0 + 1] - a.uoff[s0];
            for (int64_t t = s0 + 1; t < s1; ++t) {
                const int64_t n = a.uoff[t + 1] - a.uoff[t];
                if (n < best) {
                    best = n;
                    drv = t;
                }
            }
            keep = s == drv;
            if (FILTER && keep) {
                const u64* __restrict__ bits = a.keep_bits[j];
                if (bits) {   // (v is an atom of the snapshot: a link atom or a target, below the bitmap's end)
                    ++tested;
                    keep = (bits[v >> 6] >> (v & 63)) & 1ull;
                    if (!keep) ++rejected;
                }
            }
            for (int64_t t = s0; t < s1 && keep; ++t) {
                if (t == s) continue;
                const int64_t tb = a.uoff[t], te = a.uoff[t + 1];
                const u64 want = ((u64)t << 32) | v;
                const int64_t p = lower_bound_key(ks, tb, te, want, probes);
                keep = p < te && ks[p] == want;
            }
        }
        a.keep[i] = keep ? 1 : 0;
    }
    wave_add(a.ctr + 1, distinct);
    wave_add(a.ctr + 4, probes);
    if (FILTER) {
        wave_add(a.ctr + 6, tested);
        wave_add(a.ctr + 7, rejected);
    }
}

// out_ctr: [0] hits projected, [1] distinct values of the parts, [2] ids kept, [3] probes of the key kernel,
// [4] probes of the keep kernel, [5] targets read, [6] values tested by the filter, [7] values it rejected.
__global__ void __launch_bounds__(256) hgx_join_place(JoinArgs a) {
    if (a.stat[2]) return;
    const int64_t H = a.uoff[a.n_parts];
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ts = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = t0; i < H; i += ts)
        if (a.keep[i]) a.out_ids[a.pre[i]] = (int32_t)(a.key_sorted[i] & kMissing);
    for (int64_t j = t0; j <= a.n_queries; j += ts) a.out_off[j] = a.pre[a.uoff[a.part_off[j]]];
    if (t0 < 8) a.out_ctr[t0] = t0 == 0 ? (u64)H : t0 == 2 ? (u64)a.pre[H] : a.ctr[t0];
}

}  // namespace

void join_validate(int32_t n_queries, const int64_t* part_off, const int32_t* part_pos, int32_t flags, const char* name,
                   int32_t known_flags) {
    const std::string who = std::string(name) + ": ";
    if (n_queries < 0 || !part_off) fail(HGX_E_INVALID, who + "bad argument");
    if (flags & ~known_flags) fail(HGX_E_INVALID, who + "unknown flag");
    if (part_off[0] != 0) fail(HGX_E_INVALID, who + "part_off[0] is not 0");
    for (int32_t j = 0; j < n_queries; ++j)
        if (part_off[j + 1] < part_off[j])
            fail(HGX_E_INVALID, who + "part_off decreases at join query " + std::to_string(j));
    const int64_t np = part_off[n_queries];
    if (np > (int64_t)INT32_MAX - 2) fail(HGX_E_UNSUPPORTED, who + "too many parts");
    if (np > 0 && !part_pos) fail(HGX_E_INVALID, who + "null part_pos");
    for (int32_t j = 0; j < n_queries; ++j)
        for (int64_t s = part_off[j]; s < part_off[j + 1]; ++s)
            if (part_pos[s] < HGX_JOIN_SELF)
                fail(HGX_E_INVALID, who + "join query " + std::to_string(j) + " part " + std::to_string(s - part_off[j]) +
                                        ": bad target position " + std::to_string(part_pos[s]));
}

size_t join_temp_bytes(int64_t cap, int32_t sort_bits, hipStream_t s) {
    size_t sb = 0;
    HGX_HIP(rocprim::radix_sort_keys(nullptr, sb, (const u64*)nullptr, (u64*)nullptr, (size_t)cap, 0u,
                                     (unsigned)sort_bits, s));
    return sb;
}

void join_launch(const JoinArgs& a, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    const int grid = grid_for(a.cap, 256, 4096);
    HGX_HIP(hipMemsetAsync(a.ctr, 0, sizeof(u64) * 8, s));
    hgx_join_key<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    size_t sb = a.sort_tmp_bytes;
    HGX_HIP(rocprim::radix_sort_keys(a.sort_tmp, sb, (const u64*)a.key, a.key_sorted, (size_t)a.cap, 0u,
                                     (unsigned)a.sort_bits, s));
    if (k0) HGX_HIP(hipEventRecord(k0, s));
    if (a.keep_bits) hgx_join_keep<true><<<grid, 256, 0, s>>>(a);
    else hgx_join_keep<false><<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    if (k1) HGX_HIP(hipEventRecord(k1, s));
    sb = a.tmp_bytes;
    HGX_HIP(rocprim::exclusive_scan(a.tmp, sb, (const uint8_t*)a.keep, a.pre, (int64_t)0, (size_t)a.cap + 1,
                                    rocprim::plus<int64_t>(), s));
    hgx_join_place<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
}

}  // namespace hgx
