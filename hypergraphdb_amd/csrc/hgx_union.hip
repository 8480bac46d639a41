// hgx_union.hip -- the sorted union of the clause results of a DNF batch (hgx_pattern_batch_dnf).
//
// Replaces OrToQuery (C/query/cond2qry/OrToQuery.java:14-43) chaining UnionResults
// (C/query/impl/UnionResult.java): the ordered, duplicate-free union of the result sets of an Or's
// operands.  The operands are the clauses of the batch, already matched and placed in device memory by
// the single-pass pattern pipeline (hgx_query.hip): clause c's hits are hits[run_off[c], run_off[c+1]),
// ascending, and query q owns the clauses [clause_off[q], clause_off[q+1]) -- so its hits are one
// contiguous range made of k ascending runs.
//
// GPU formulation: a lane per clause hit over the flat hit space, no atomics deciding
// order.
//   hgx_union_keep   -- hit e of clause c is kept iff no EARLIER clause of its query contains the same
//        id (a binary search in each earlier run): every distinct id of a query is kept exactly once;
//   the scan         -- pre = exclusive prefix sum of the keep flags over the flat space (rocPRIM, sized
//        from the workspace capacity: the hit total is known on the device only);
//   hgx_union_place  -- a kept id x goes to qoff[q] + sum over the query's runs r of
//        (pre[start_r + lower_bound(r, x)] - pre[start_r]) = qoff[q] + the kept ids of q below x, with
//        qoff[q] = pre[first hit of q]; the same kernel writes qoff;
//   hgx_union_publish -- the statistics of the batch into the mapped result area.
// All of them read the hit total and the overflow flag of the clause stage from device memory and do
// nothing after an overflow, so no host round trip sits between the clause stage and the union.
#include <rocprim/device/device_scan.hpp>

#include "hgx_internal.h"

namespace hgx {

namespace {

typedef unsigned long long u64;

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

// first p in [b, e) with a[p] >= v (e when none)
__device__ __forceinline__ int64_t lower_bound_id(const int32_t* __restrict__ a, int64_t b, int64_t e, int32_t v,
                                                  u64& probes) {
    while (b < e) {
        const int64_t mid = (b + e) >> 1;
        ++probes;
        if (a[mid] < v) b = mid + 1;
        else e = mid;
    }
    return b;
}

__device__ __forceinline__ void wave_add(u64* p, u64 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(p, v);
}

__global__ void __launch_bounds__(256) hgx_union_keep(UnionArgs a) {
    if (a.stat[2]) return;   // the clause stage overflowed its workspace: the host grows it and runs again
    const int64_t H = a.run_off[a.n_clauses];
    u64 probes = 0, runs = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = upper_bound_off(a.run_off, (int64_t)a.n_clauses + 1, e) - 1;
        const int64_t q = upper_bound_off(a.clause_off, (int64_t)a.n_queries + 1, c) - 1;
        const int32_t x = a.hits[e];
        bool keep = true;
        for (int64_t r = a.clause_off[q]; r < c && keep; ++r) {
            const int64_t b = a.run_off[r], en = a.run_off[r + 1];
            ++runs;
            if (b == en) continue;
            const int64_t p = lower_bound_id(a.hits, b, en, x, probes);
            if (p < en && a.hits[p] == x) keep = false;
        }
        a.keep[e] = keep ? 1 : 0;
    }
    wave_add(a.ctr + 0, probes);
    wave_add(a.ctr + 1, runs);
}

__global__ void __launch_bounds__(256) hgx_union_place(UnionArgs a) {
    if (a.stat[2]) return;
    const int64_t H = a.run_off[a.n_clauses];
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ts = (int64_t)gridDim.x * blockDim.x;
    u64 probes = 0, runs = 0;
    for (int64_t e = t0; e < H; e += ts) {
        if (!a.keep[e]) continue;
        const int64_t c = upper_bound_off(a.run_off, (int64_t)a.n_clauses + 1, e) - 1;
        const int64_t q = upper_bound_off(a.clause_off, (int64_t)a.n_queries + 1, c) - 1;
        const int32_t x = a.hits[e];
        const int64_t c0 = a.clause_off[q], c1 = a.clause_off[q + 1];
        int64_t slot = a.pre[a.run_off[c0]];
        for (int64_t r = c0; r < c1; ++r) {
            const int64_t b = a.run_off[r], en = a.run_off[r + 1];
            ++runs;
            if (b == en) continue;
            const int64_t p = r == c ? e : lower_bound_id(a.hits, b, en, x, probes);
            slot += a.pre[p] - a.pre[b];
        }
        a.out_ids[slot] = x;
    }
    for (int64_t q = t0; q <= a.n_queries; q += ts) a.out_off[q] = a.pre[a.run_off[a.clause_off[q]]];
    wave_add(a.ctr + 2, probes);
    wave_add(a.ctr + 3, runs);
}

// out_stat: [0] chunks, [1] candidates, [2] overflow, [4] / [5] bad / unsupported clause of the clause
// stage; [3] ids kept, [6] clause hits; out_ctr: the four probe / run counters.
__global__ void __launch_bounds__(64) hgx_union_publish(UnionArgs a) {
    if (threadIdx.x != 0) return;
    const bool over = a.stat[2] != 0;
    const int64_t H = over ? 0 : a.run_off[a.n_clauses];
    a.out_stat[0] = a.stat[0];
    a.out_stat[1] = a.stat[1];
    a.out_stat[2] = a.stat[2];
    a.out_stat[3] = over ? 0 : a.pre[H];
    a.out_stat[4] = a.stat[4];
    a.out_stat[5] = a.stat[5];
    a.out_stat[6] = H;
    for (int k = 0; k < 4; ++k) a.out_ctr[k] = a.ctr[k];
}

}  // namespace

size_t union_temp_bytes(int64_t cap, hipStream_t s) {
    size_t sb = 0;
    HGX_HIP(rocprim::exclusive_scan(nullptr, sb, (const uint8_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)cap + 1,
                                    rocprim::plus<int64_t>(), s));
    return sb;
}

void union_launch(const UnionArgs& a, hipStream_t s) {
    const int grid = grid_for(a.cap, 256, 4096);
    HGX_HIP(hipMemsetAsync(a.ctr, 0, sizeof(u64) * 4, s));
    hgx_union_keep<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    size_t sb = a.tmp_bytes;
    HGX_HIP(rocprim::exclusive_scan(a.tmp, sb, (const uint8_t*)a.keep, a.pre, (int64_t)0, (size_t)a.cap + 1,
                                    rocprim::plus<int64_t>(), s));
    hgx_union_place<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    hgx_union_publish<<<1, 64, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
}

}  // namespace hgx
